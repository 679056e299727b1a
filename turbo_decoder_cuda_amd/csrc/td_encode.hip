// td_encode.hip -- the batched LTE turbo encoder (td_encode_device) and the CRC-24 attach / check
// (td_crc_attach, td_crc_check) on device-resident bits.  The arithmetic is td_encode_core.h's, which the
// host tests run as a plain program; this file is the data path round it.
//
// Encoder: one workgroup of 256 threads takes one codeword at a time (grid-stride over the batch), and no
// thread walks the trellis -- the constituent code is a prefix XOR at stride 7 (td_encode_core.h):
//   1  the info row is read coalesced and packed to bits in LDS (u1): eight bytes a lane and one byte of
//      bits each where the row is 8-byte aligned, else a byte a lane and a wave's ballot as a 64-bit word
//   2  the second encoder's input u2[i] = u1[pi(i)] is gathered from that bit array with the QPP table,
//      which the workgroup keeps in LDS as 16-bit entries (read from the handle's table once a workgroup):
//      a thread reads eight entries at once and gathers a byte of u2
//   3  one thread per word (at most 157): the in-word prefixes of both numerators of both encoders, then
//      an exclusive XOR scan of the 28 carry bits over the words -- shuffles inside a wave, the waves'
//      totals through LDS -- and the words of a (for the tails) and p1, p2
//   4  eight info bits a thread: their 24 (x, p1, p2) bytes go to the stage in LDS as six dwords; the thread
//      of the last byte adds the twelve tail bytes
//   5  the stage leaves as 16-byte pieces, every wave one contiguous kilobyte a store
// Rows are only byte-aligned in general (odd K, or 3K + 12 no multiple of 16 with B > 1).  Input: the two
// forms of step 1 write the same bits.  Output: the stage is shifted so that 16-byte pieces of the
// destination are 16-byte aligned in LDS (row_split), the few bytes before the first and after the last
// boundary go singly, and a row that is not even dword-aligned funnels its pieces by one to three bytes:
// one path for every alignment.  The bytes do not depend on the alignment (tests/test_gpu_encode.py).
//
// LDS per workgroup (K = 6144: 12 + 4.5 + 18.1 = 34.6 KiB, four workgroups a CU; K = 10000: 56.2 KiB, two).
#include <hip/hip_runtime.h>

#include "td_encode.h"
#include "td_encode_core.h"

namespace td {

namespace {

using namespace enc;

constexpr int kEncThreads = 256, kEncWaves = kEncThreads / 64;
constexpr int kEncBatch = 12;   // words a wave has in flight while it reads the row (K = 6144: 24 a wave, two batches)
static_assert(kMaxWords <= kEncThreads, "one thread per word");

// byte offsets of the encoder's LDS arrays, all 16-byte aligned
struct EncLds {
    int pi16, u1, u2, a1, a2, p1, p2, tot, stage, total;
};
__host__ __device__ inline EncLds enc_lds(int K)
{
    auto up = [](int v) { return (v + 15) & ~15; };
    const int words = up(8 * words_for(K));
    EncLds l;
    l.pi16 = 0;
    l.u1 = up(2 * (K + 7));   // padded to whole groups of eight
    l.u2 = l.u1 + words;
    l.a1 = l.u2 + words;
    l.a2 = l.a1 + words;
    l.p1 = l.a2 + words;
    l.p2 = l.p1 + words;
    l.tot = l.p2 + words;
    l.stage = l.tot + 16;
    l.total = l.stage + up(4 * stage_dwords(3 * K + 12));
    return l;
}

extern __shared__ __attribute__((aligned(16))) unsigned char td_enc_smem[];

__global__ __launch_bounds__(kEncThreads) void encode_kernel(EncParams p)
{
    const int K = p.K, nW = words_for(K), n = 3 * K + 12;
    const EncLds L = enc_lds(K);
    uint16_t* pi16 = reinterpret_cast<uint16_t*>(td_enc_smem + L.pi16);
    uint64_t* u1 = reinterpret_cast<uint64_t*>(td_enc_smem + L.u1);
    uint64_t* u2 = reinterpret_cast<uint64_t*>(td_enc_smem + L.u2);
    uint64_t* a1 = reinterpret_cast<uint64_t*>(td_enc_smem + L.a1);
    uint64_t* a2 = reinterpret_cast<uint64_t*>(td_enc_smem + L.a2);
    uint64_t* p1 = reinterpret_cast<uint64_t*>(td_enc_smem + L.p1);
    uint64_t* p2 = reinterpret_cast<uint64_t*>(td_enc_smem + L.p2);
    uint32_t* tot = reinterpret_cast<uint32_t*>(td_enc_smem + L.tot);
    uint32_t* stage = reinterpret_cast<uint32_t*>(td_enc_smem + L.stage);
    const uint32_t* u1w = reinterpret_cast<const uint32_t*>(u1);
    uint8_t* u1b = reinterpret_cast<uint8_t*>(u1);   // the same bits by the byte
    uint8_t* u2b = reinterpret_cast<uint8_t*>(u2);
    const uint8_t* p1b = reinterpret_cast<const uint8_t*>(p1);
    const uint8_t* p2b = reinterpret_cast<const uint8_t*>(p2);
    const int nB = (K + 7) >> 3;   // bytes of a row's bit array

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 8 * nB; i += kEncThreads) pi16[i] = i < K ? (uint16_t)p.pi[i] : (uint16_t)0;   // K <= 10000 < 2^16

    for (size_t b = blockIdx.x; b < (size_t)p.B; b += gridDim.x) {
        const uint8_t* in = p.info + b * (size_t)K;
        uint8_t* out = p.coded + b * (size_t)n;

        // 1: bytes -> bits.  An 8-byte aligned row: eight bytes a lane (a 512-byte piece a wave and load), up to
        // four loads a lane in flight, a byte of the bit array each; the K % 8 last bytes go with the last lane.
        // Any other row: a byte a lane, a wave's ballot is a word, kEncBatch loads in flight.
        if ((reinterpret_cast<uintptr_t>(in) & 7u) == 0) {
            const int nG = K >> 3;
            for (int j0 = tid; j0 < nG; j0 += 4 * kEncThreads) {
                uint2 v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = j0 + kEncThreads * k;
                    v[k] = j < nG ? *reinterpret_cast<const uint2*>(in + 8 * (size_t)j) : make_uint2(0, 0);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = j0 + kEncThreads * k;
                    if (j < nG) u1b[j] = (uint8_t)nonzero8(v[k].x, v[k].y);
                }
            }
            if (tid == kEncThreads - 1 && (K & 7)) {
                uint32_t m = 0;
                for (int i = 8 * nG; i < K; ++i) m |= (in[i] != 0 ? 1u : 0u) << (i & 7);
                u1b[nG] = (uint8_t)m;
            }
            if (tid < 8 * nW - nB) u1b[nB + tid] = 0;   // the last word's bytes past the row
        } else {
            for (int w0 = wave; w0 < nW; w0 += kEncWaves * kEncBatch) {
                uint8_t v[kEncBatch];
#pragma unroll
                for (int k = 0; k < kEncBatch; ++k) {
                    const int i = 64 * (w0 + kEncWaves * k) + lane;
                    v[k] = i < K ? in[i] : (uint8_t)0;
                }
#pragma unroll
                for (int k = 0; k < kEncBatch; ++k) {
                    const int w = w0 + kEncWaves * k;
                    const uint64_t m = __ballot(v[k] != 0);
                    if (lane == 0 && w < nW) u1[w] = m;
                }
            }
        }
        __syncthreads();   // (the first time round: pi16 as well)

        // 2: u2 = u1 o pi, a byte of u2 a thread: eight table entries in one read, eight gathered bits
        for (int j = tid; j < nB; j += kEncThreads) {
            const Vec16 t = *reinterpret_cast<const Vec16*>(pi16 + 8 * j);
            uint32_t acc = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t s = (t.v[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
                acc |= ((u1w[s >> 5] >> (s & 31)) & 1u) << k;
            }
            const int valid = K - 8 * j;   // the entries past K are padding (0): their bits stay out
            if (valid < 8) acc &= (1u << valid) - 1u;
            u2b[j] = (uint8_t)acc;
        }
        if (tid < 8 * nW - nB) u2b[nB + tid] = 0;
        __syncthreads();

        // 3: a word a thread, and the carry scan
        WordLocal l1{0, 0, 0}, l2{0, 0, 0};
        if (tid < nW) {
            l1 = word_local(u1[tid], tid ? u1[tid - 1] : 0, tid);
            l2 = word_local(u2[tid], tid ? u2[tid - 1] : 0, tid);
        }
        const uint32_t q = l1.q | (l2.q << 14);
        uint32_t inc = q;   // inclusive XOR scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(inc, d);
            if (lane >= d) inc ^= t;
        }
        if (lane == 63) tot[wave] = inc;
        __syncthreads();
        uint32_t r = inc ^ q;
        for (int v = 0; v < wave; ++v) r ^= tot[v];
        if (tid < nW) {
            uint64_t a, pp;
            word_finish(l1, r & 0x3FFFu, tid, a, pp);
            a1[tid] = a, p1[tid] = pp;
            word_finish(l2, r >> 14, tid, a, pp);
            a2[tid] = a, p2[tid] = pp;
        }
        __syncthreads();

        // 4: the (x, p1, p2) bytes and the tails, staged where row_split wants them
        const RowSplit sp = row_split(reinterpret_cast<uintptr_t>(out), n);
        for (int j = tid; j < nB; j += kEncThreads) {   // eight info bits: 24 bytes, six dwords at lane stride 6
            uint32_t d[6];
            pack24(u1b[j], p1b[j], p2b[j], d);
            uint32_t* s = stage + sp.s4 + 6 * j;
#pragma unroll
            for (int k = 0; k < 6; ++k) s[k] = d[k];
        }
        uint8_t* stage8 = reinterpret_cast<uint8_t*>(stage) + 4 * sp.s4;   // row byte x
        if (tid == (nB - 1) % kEncThreads) {   // after this thread's own last byte, whose 24 bytes may reach past 3K
            uint8_t t6[6];
            tail6(row_bit(a1, K - 1), row_bit(a1, K - 2), row_bit(a1, K - 3), t6);
#pragma unroll
            for (int j = 0; j < 6; ++j) stage8[3 * K + j] = t6[j];
            tail6(row_bit(a2, K - 1), row_bit(a2, K - 2), row_bit(a2, K - 3), t6);
#pragma unroll
            for (int j = 0; j < 6; ++j) stage8[3 * K + 6 + j] = t6[j];
        }
        __syncthreads();

        // 5: out
        if (tid < sp.head) out[tid] = stage8[tid];
        for (int j = tid; j < sp.nvec; j += kEncThreads) {
            const Vec16 v = stage_vec(stage, sp, j);
            *reinterpret_cast<Vec16*>(out + sp.head + 16 * (size_t)j) = v;
        }
        const int done = sp.head + 16 * sp.nvec;
        if (tid < sp.tail) out[done + tid] = stage8[done + tid];
        // no barrier: the next codeword's writes to u1, u2, tot and the stage each come after a barrier that
        // every thread reaches only when it is done with this codeword's reads of them
    }
}

// CRC-24: a wave takes a row at a time, the lanes consecutive bytes; the syndrome table sits in LDS (read
// once a workgroup).  attach XORs syn[i + 24] over the payload's set bits and writes the 24 CRC bytes; check
// XORs syn[i] over all K.
constexpr int kCrcThreads = 256, kCrcWaves = kCrcThreads / 64;

extern __shared__ __attribute__((aligned(16))) unsigned char td_crc_smem[];

template <bool ATTACH>
__global__ __launch_bounds__(kCrcThreads) void crc_kernel(CrcParams p, uint8_t* bits, uint32_t* rem)
{
    uint32_t* syn = reinterpret_cast<uint32_t*>(td_crc_smem);
    const int K = p.K, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < K; i += kCrcThreads) syn[i] = p.syn[i];
    __syncthreads();
    const int n = ATTACH ? K - 24 : K, off = ATTACH ? 24 : 0;
    for (size_t b = (size_t)blockIdx.x * kCrcWaves + wave; b < (size_t)p.B; b += (size_t)gridDim.x * kCrcWaves) {
        uint8_t* row = bits + b * (size_t)K;
        uint32_t acc = 0;
#pragma unroll 8
        for (int i = lane; i < n; i += 64) acc ^= crc_term(row[i], syn[i + off]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc ^= __shfl_xor(acc, d);
        if constexpr (ATTACH) {
            if (lane < 24) row[K - 24 + lane] = crc_out_bit(acc, lane);
        } else {
            if (lane == 0) rem[b] = acc;
        }
    }
}

}  // namespace

hipError_t launch_encode(const EncParams& p, hipStream_t st)
{
    const EncLds L = enc_lds(p.K);
    const int per_cu = (160 * 1024) / L.total;   // workgroups a CU holds
    const long long cap = (long long)(p.cus > 0 ? p.cus : 256) * (per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu);
    const unsigned grid = (unsigned)(p.B < cap ? p.B : cap);
    hipLaunchKernelGGL(encode_kernel, dim3(grid), dim3(kEncThreads), (size_t)L.total, st, p);
    return hipGetLastError();
}

namespace {

unsigned crc_grid(const CrcParams& p)
{
    const long long need = ((long long)p.B + kCrcWaves - 1) / kCrcWaves, cap = (long long)(p.cus > 0 ? p.cus : 256) * 4;
    return (unsigned)(need < cap ? need : cap);
}

}  // namespace

hipError_t launch_crc_attach(const CrcParams& p, uint8_t* d_bits, hipStream_t st)
{
    hipLaunchKernelGGL(crc_kernel<true>, dim3(crc_grid(p)), dim3(kCrcThreads), (size_t)p.K * sizeof(uint32_t), st, p, d_bits,
                       static_cast<uint32_t*>(nullptr));
    return hipGetLastError();
}

hipError_t launch_crc_check(const CrcParams& p, const uint8_t* d_bits, uint32_t* d_rem, hipStream_t st)
{
    hipLaunchKernelGGL(crc_kernel<false>, dim3(crc_grid(p)), dim3(kCrcThreads), (size_t)p.K * sizeof(uint32_t), st, p,
                       const_cast<uint8_t*>(d_bits), d_rem);
    return hipGetLastError();
}

}  // namespace td
