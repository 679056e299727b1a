// tb_core_host.cpp -- csrc/td_tb_core.h as a stand-alone host program (ASan + UBSan; tests/test_tb_host.py):
// the plan and the index arithmetic the gfx950 kernels of td_tb.hip use -- element -> block / offset / source.
//
//   tb_core_host in.bin out.bin
// in:  int32 count, then `count` triples (A, G, NlQm)
// out: int32 words per triple, in this order
//   the plan's nine fields
//   per block r: K_r, block_start, block_row(r, n = 2, N = 5), then (kind, idx) of seg_src for every offset
//   (r, i) of locate for every bit s < B
//   E_lo, E_hi, n_lo; per block r: e_start, e_size; (r, k) of e_locate for every g < G
#include <cstdint>
#include <cstdio>
#include <vector>

#include "td_tb_core.h"

using namespace td::tb;

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t count = 0;
    if (std::fread(&count, 4, 1, f) != 1 || count < 0) return 2;
    std::vector<int32_t> in(3 * (size_t)count);
    if (!in.empty() && std::fread(in.data(), 4, in.size(), f) != in.size()) return 2;
    std::fclose(f);

    std::vector<int32_t> out;
    for (int c = 0; c < count; ++c) {
        const int A = in[3 * c], G = in[3 * c + 1], NlQm = in[3 * c + 2];
        Plan p;
        if (!plan(A, p)) return 3;
        for (int v : {p.A, p.B, p.L, p.C, p.K_plus, p.K_minus, p.C_plus, p.C_minus, p.F}) out.push_back(v);
        for (int r = 0; r < p.C; ++r) {
            out.push_back(block_k(p, r));
            out.push_back(block_start(p, r));
            out.push_back((int32_t)block_row(p, r, 2, 5));
            for (int i = 0; i < block_k(p, r); ++i) {
                const SegSrc s = seg_src(p, r, i);
                out.push_back(s.kind);
                out.push_back(s.idx);
            }
        }
        for (int s = 0; s < p.B; ++s) {
            const Loc l = locate(p, s);
            out.push_back(l.r);
            out.push_back(l.i);
        }
        RmSizes sz;
        if (!rm_sizes(p.C, G, NlQm, sz)) return 4;
        for (int v : {sz.E_lo, sz.E_hi, sz.n_lo}) out.push_back(v);
        for (int r = 0; r < p.C; ++r) {
            out.push_back((int32_t)e_start(sz, r));
            out.push_back(e_size(sz, r));
        }
        for (long long g = 0; g < G; ++g) {
            const Loc l = e_locate(sz, g);
            out.push_back(l.r);
            out.push_back(l.i);
        }
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    if (!out.empty() && std::fwrite(out.data(), 4, out.size(), f) != out.size()) return 2;
    std::fclose(f);
    return 0;
}
