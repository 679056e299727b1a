// frontend_core_host.cpp -- csrc/td_demap_core.h as a stand-alone host program (tests/test_frontend_host.py,
// built with ASan + UBSan): the demappers, the LLR conversion and the value source the fused
// de-rate-matching kernels read, through the same routines the gfx950 kernels call.
//
//   frontend_core_host <in> <out>
//   in:  int32 mode, then
//        mode 0 (demap):   int32 M, nsym; double Kf; double yi[nsym], yq[nsym]
//             out: double llr[nsym * M] -- demod_symbol<M> (M = 1: demod_bpsk), as td_demodulate; the program
//                  fails if demod_bit<M> gives another double for any bit
//        mode 1 (convert): int32 n, 0; double steps_per_unit; double x[n]
//             out: double copy[n]; float f[n]; int8 q[n]
//        mode 2 (the definition of td_demod_dematch): int32 M, prec (0 f64, 1 f32, 2 int8), B, E, nout, acc;
//             double Kf, steps_per_unit; int32 idx[E]; double yi[B][E / M], yq[B][E / M]; T prior[B][nout]
//             out: T llr[B][nout] -- position idx[k] takes e[b][k] in ascending k, onto prior (acc) or 0; int8
//                  saturates to +-127 after every addition and reads a prior -128 as -127
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "td_demap_core.h"

static std::vector<uint8_t> slurp(const char* path)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::perror(path); std::exit(2); }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

struct Reader {
    const std::vector<uint8_t>& v;
    size_t at = 0;
    template <typename T>
    std::vector<T> take(size_t n)
    {
        if (at + n * sizeof(T) > v.size()) { std::fprintf(stderr, "input too short\n"); std::exit(2); }
        std::vector<T> r(n);
        if (n) std::memcpy(r.data(), v.data() + at, n * sizeof(T));
        at += n * sizeof(T);
        return r;
    }
};

template <typename T>
static void put(FILE* f, const std::vector<T>& v)
{
    if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { std::perror("write"); std::exit(2); }
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

template <int M>
static std::vector<double> demap(const std::vector<double>& yi, const std::vector<double>& yq, double Kf)
{
    std::vector<double> out(yi.size() * M);
    for (size_t s = 0; s < yi.size(); ++s) {
        double o[M];
        if (M == 1)
            o[0] = td::demod_bpsk(yi[s], yq[s], Kf);
        else
            td::demod_symbol<M>(yi[s], yq[s], Kf, o);
        for (int b = 0; b < M; ++b) {
            out[s * M + b] = o[b];
            if (!same_bits(o[b], td::demod_bit<M>(yi[s], yq[s], Kf, b))) {
                std::fprintf(stderr, "M = %d symbol %zu bit %d: demod_bit differs from demod_symbol\n", M, s, b);
                std::exit(3);
            }
        }
    }
    return out;
}

static void add(double& acc, double v) { acc += v; }
static void add(float& acc, float v) { acc += v; }
static void add(int8_t& acc, int8_t v)
{
    int a = acc < -127 ? -127 : acc;
    a += v;
    acc = (int8_t)(a > 127 ? 127 : a < -127 ? -127 : a);
}

template <int M, typename T>
static void definition(Reader& r, FILE* f, int B, int E, int nout, int acc, double Kf, double spu)
{
    const std::vector<int32_t> idx = r.take<int32_t>(E);
    const size_t nsym = (size_t)E / M;
    const std::vector<double> yi = r.take<double>(B * nsym), yq = r.take<double>(B * nsym);
    std::vector<T> out = r.take<T>((size_t)B * nout);
    if (!acc) std::fill(out.begin(), out.end(), T(0));
    const td::DemapSrc<M, T> src{yi.data(), yq.data(), nsym, Kf, spu};
    for (int b = 0; b < B; ++b) {
        const auto e = src.row(b);
        T* o = out.data() + (size_t)b * nout;
        for (int k = 0; k < E; ++k) {
            if (idx[k] < 0 || idx[k] >= nout) { std::fprintf(stderr, "idx out of range\n"); std::exit(2); }
            add(o[idx[k]], e[k]);   // (a position nothing selects keeps its byte, a prior -128 included)
        }
    }
    put(f, out);
}

template <int M>
static void definition_m(Reader& r, FILE* f, int prec, int B, int E, int nout, int acc, double Kf, double spu)
{
    if (prec == 0) definition<M, double>(r, f, B, E, nout, acc, Kf, spu);
    else if (prec == 1) definition<M, float>(r, f, B, E, nout, acc, Kf, spu);
    else definition<M, int8_t>(r, f, B, E, nout, acc, Kf, spu);
}

#define BY_M(M, call)                                                                  \
    switch (M) {                                                                       \
        case 1: call(1); break;                                                        \
        case 2: call(2); break;                                                        \
        case 3: call(3); break;                                                        \
        case 4: call(4); break;                                                        \
        case 6: call(6); break;                                                        \
        default: std::fprintf(stderr, "bad M\n"); return 2;                            \
    }

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const std::vector<uint8_t> in = slurp(argv[1]);
    Reader r{in};
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) { std::perror(argv[2]); return 2; }
    const int mode = r.take<int32_t>(1)[0];
    if (mode == 0) {
        const std::vector<int32_t> h = r.take<int32_t>(2);
        const int M = h[0], nsym = h[1];
        const double Kf = r.take<double>(1)[0];
        const std::vector<double> yi = r.take<double>(nsym), yq = r.take<double>(nsym);
#define DEMAP(m) put(f, demap<m>(yi, yq, Kf))
        BY_M(M, DEMAP)
    } else if (mode == 1) {
        const int n = r.take<int32_t>(2)[0];
        const double spu = r.take<double>(1)[0];
        const std::vector<double> x = r.take<double>(n);
        std::vector<double> c(n);
        std::vector<float> fl(n);
        std::vector<int8_t> q(n);
        for (int i = 0; i < n; ++i) {
            c[i] = td::llr_to<double>(x[i], spu);
            fl[i] = td::llr_to<float>(x[i], spu);
            q[i] = td::llr_to<int8_t>(x[i], spu);
        }
        put(f, c), put(f, fl), put(f, q);
    } else if (mode == 2) {
        const std::vector<int32_t> h = r.take<int32_t>(6);
        const int M = h[0], prec = h[1], B = h[2], E = h[3], nout = h[4], acc = h[5];
        const std::vector<double> d = r.take<double>(2);
        if (B < 0 || E < 1 || nout < 1 || prec < 0 || prec > 2 || M < 1 || E % M) return 2;
#define DEFN(m) definition_m<m>(r, f, prec, B, E, nout, acc, d[0], d[1])
        BY_M(M, DEFN)
    } else {
        return 2;
    }
    return std::fclose(f) == 0 ? 0 : 2;
}
