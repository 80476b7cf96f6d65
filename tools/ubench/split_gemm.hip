// split_gemm.hip -- stand-alone micro-benchmark of ONE 512 x 512 split-operand linear of the fused fp32-class network
// (pnr::eval_split_kernel, pixel-nerf_amd/csrc/pnr_split.hip), VERDICT r04 "next" item 2.
//
// What it settles: eval_split_kernel re-streams the 10.8 MB (head + tail) weight set from L2 for every 64-point tile -- 2 KiB of
// weight fragments per 3 JT MFMAs -- and the only lever on bytes per MFMA is JT, the number of 32-point column tiles a fragment
// feeds.  LDS pins the shipped form at JT = 2 (two 66.5 KB operand images).  The candidate is a ONE-wave-per-SIMD, 512-register
// form: 4 waves x 128 features (IT = 4), JT = 3 or 4, accumulators in AGPRs, operand images holding one K half at a time.  This
// program times the GEMM loop of both forms on the real footprint (a 10 x 512 x 512 (head, tail) stream per workgroup pass, so
// the per-XCD L2 behaves as in the product), with the issue order of the product loop, and nothing else of the network:
// if the wide form's loop is not >= 10 % faster per point here, no integration of it can be.
//
//   form          waves  IT JT  regs/lane (acc + ring + B)   LDS image (head + tail)       extras
//   shipped         8     2  2  64 [+64] + 64 + 32           64 pts x 512 K  = 133 KB      1 barrier per GEMM
//   wide-96         4     4  3  192 [+192] + 64|128 + 48     96 pts x 256 K  = 101 KB      3 barriers per GEMM (K halves)
//   wide-128        4     4  4  256 + 64|128 + 64            128 pts x 256 K = 135 KB      3 barriers per GEMM, PARK: the residual
//                                                                                          stream x leaves the registers for an
//                                                                                          L2-resident scratch around every fc_0
//                                                                                          (256 KB out + 256 KB in per block)
// [+..] = a second accumulator set kept live (x next to net), as the product holds it.
//
// Second question (round 7): the MFMA SHAPE.  The chip is power-limited under this loop (1.82 of 2.4 GHz), and the clock it holds can
// depend on the shape at equal cycles per FLOP, so only wall time on RANDOM data ranks the two.  The '16x16x32' form has the
// shipped footprint -- 8 waves, 64 features x 64 points per wave, both images in LDS, 16 KiB of ring per wave, 3 MFMAs per
// product -- on v_mfma_f32_16x16x32_f16: 4 feature tiles x 4 point tiles of 16, one ring step = one K = 32 step (4 tiles x 1 KiB
// per blob, ring of 2), and the B fragment pair of ONE point tile fetched just in time (two pairs in rotation, 16 registers;
// each pair feeds 12 MFMAs).
//
//   form          waves  tiles     regs/lane (acc + ring + B)   LDS image (head + tail)
//   16x16x32        8    4 x 4     64 [+64] + 64 + 16           64 pts x 512 K  = 133 KB      1 barrier per GEMM
//
// Build + run (one MI355X):  hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench/split_gemm.hip -o /tmp/split_gemm && /tmp/split_gemm
//   split_gemm [reps [rounds]]        the shape gate: shipped and 16x16x32 (with and without the weight stream), interleaved in one
//                                     process for `rounds` rounds; per form median and min us per launch, the rate relative to
//                                     shipped, and the spread of shipped against itself.  Before any timing ONE GEMM of each form
//                                     is checked on one 64-point tile against a host reference (the fragment maps, on the device).
//   split_gemm --wide [reps]          the round-5 table: one line per wide form -- us per launch, points x GEMMs per second,
//                                     executed MFMA TFLOP/s (3 MFMAs per product), and the rate relative to the shipped form
//                                     (register counts: tools/kernel_regs.py on the binary).
//   -DUB_STAMP: a diagnostic build that stamps the shader clock and the 100 MHz real-time clock around each workgroup's tile loop
//   (into a buffer of their own) and prints the in-kernel clock and the cycles per launch next to the wall time.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define CK(x)                                                                                      \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } \
    } while (0)

constexpr int D = 512, KS = D / 16;  // 32 k-steps of 16
constexpr int NG = 10;               // GEMMs per tile pass: the ten 512 x 512 linears of a folded single-view network

__device__ __forceinline__ f32x16 mf(h8 a, h8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mf16(h8 a, h8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

// element i of the two operand images (head image, then tail image, rows of ROW bytes): something finite and non-trivial,
// both signs, the same on the device and in the host reference
__host__ __device__ inline _Float16 image_value(int i) { return (_Float16)(((i * 37 + 11) % 61) * (1.f / 64.f) - 0.45f); }

// After the ring's first fill, which hipcc issues in an order of its own: with those requests still counted, the header of the
// first GEMM loop (one instruction for the way in and for the back edge) becomes `s_waitcnt vmcnt(0)` and drains the ring at
// every body (tools/loop_header_waits.py).  Waiting once here leaves the back edge's count as the only one.
__device__ __forceinline__ void ring_landed() { __builtin_amdgcn_s_waitcnt(0x0F70); }  // vmcnt(0)

// -DUB_STAMP only: {shader clock, 100 MHz real-time clock} x {before, after} the tile loop, one record per workgroup
__device__ __forceinline__ void stamp(unsigned long long *__restrict__ stamps, int which) {
#ifdef UB_STAMP
    if (threadIdx.x == 0) {
        stamps[(size_t)blockIdx.x * 4 + 2 * which] = __builtin_amdgcn_s_memtime();
        stamps[(size_t)blockIdx.x * 4 + 2 * which + 1] = __builtin_amdgcn_s_memrealtime();
    }
#else
    (void)stamps;
    (void)which;
#endif
}

// NWV waves, wave w owns IT feature tiles of 32; JT point tiles of 32.  KHALF: the LDS images hold 256 of the 512 K (two extra
// barriers per GEMM stand for the second half's write phase).  NACC accumulator sets alternate GEMM by GEMM (x / net).
// PARK: after every second GEMM the accumulators make a round trip through a per-workgroup global scratch (the residual stream
// parked around fc_0).  LOADS = false: the ring is never refilled (upper bound without the weight stream).
// CHECK: the workgroup stops after its first GEMM and writes that GEMM's accumulators to chk[thread][it][jt][r].
template <int NWV, int IT, int JT, int RING, int NACC, bool KHALF, bool PARK, bool LOADS, bool CHECK = false>
__global__ void __launch_bounds__(NWV * 64) gemm_ub(const char *__restrict__ wstream, size_t tail_delta, float *__restrict__ out,
                                                    f32x4 *__restrict__ park_ws, float *__restrict__ chk,
                                                    unsigned long long *__restrict__ stamps, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int MT = JT * 32;
    constexpr int KIMG = KHALF ? D / 2 : D;
    constexpr int ROW = KIMG * 2 + 16;  // 16-byte pad: conflict-free ds_read_b128 (odd number of 16-byte slots per row)
    constexpr int LO_DELTA = MT * ROW;
    constexpr int KSTEPS_IMG = KIMG / 16;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pl = lane & 31, h = lane >> 5;
    for (int i = tid; i < 2 * MT * ROW / 2; i += NWV * 64) reinterpret_cast<_Float16 *>(smem)[i] = image_value(i);
    __syncthreads();

    const size_t wave_bytes = (size_t)NG * KS * IT * 1024;
    const char *base_h = wstream + (size_t)wv * wave_bytes + lane * 16;
    const char *base_l = base_h + tail_delta;
    h8 rh[RING][IT], rl[RING][IT];
#pragma unroll
    for (int j = 0; j < RING; ++j)
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            rh[j][it] = *reinterpret_cast<const h8 *>(base_h + (size_t)(j * IT + it) * 1024);
            rl[j][it] = *reinterpret_cast<const h8 *>(base_l + (size_t)(j * IT + it) * 1024);
        }
    int pf = RING;  // next k-step (of NG * KS) to prefetch
    ring_landed();

    f32x16 acc[NACC][IT][JT];
#pragma unroll
    for (int a = 0; a < NACC; ++a)
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
            for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[a][it][jt][r] = 0.f;

    const uint32_t b0 = pl * ROW + h * 16;
    float sink = 0.f;

    auto gemm = [&](f32x16 (&c)[IT][JT]) {
#pragma unroll 1
        for (int half = 0; half < (KHALF ? 2 : 1); ++half) {
            if (KHALF) {  // the half's write phase is published / the previous half's readers are done
                __syncthreads();
                if (half == 1) __syncthreads();
            } else {
                __syncthreads();
            }
            h8 bh[2][JT], bl[2][JT];
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
                bh[0][jt] = *reinterpret_cast<const h8 *>(smem + b0 + jt * 32 * ROW);
                bl[0][jt] = *reinterpret_cast<const h8 *>(smem + b0 + jt * 32 * ROW + LO_DELTA);
            }
            uint32_t bk = b0;
#pragma unroll 1
            for (int body = 0; body < KSTEPS_IMG / RING; ++body) {
                const size_t pfo = (size_t)pf * (IT * 1024);
#pragma unroll
                for (int j = 0; j < RING; ++j) {
                    const int cur = j & 1;
                    const bool lastk = (j == RING - 1) && (body == KSTEPS_IMG / RING - 1);
                    const uint32_t nx = lastk ? b0 : bk + (j + 1) * 32;  // (after the last k-step: step 0 again, read and dropped)
#pragma unroll
                    for (int jt = 0; jt < JT; ++jt) {
                        bh[cur ^ 1][jt] = *reinterpret_cast<const h8 *>(smem + nx + jt * 32 * ROW);
                        bl[cur ^ 1][jt] = *reinterpret_cast<const h8 *>(smem + nx + jt * 32 * ROW + LO_DELTA);
                    }
                    h8 ah[IT], al[IT];
#pragma unroll
                    for (int it = 0; it < IT; ++it) { ah[it] = rh[j][it]; al[it] = rl[j][it]; }
                    if constexpr (RING == 1) {
                        // just-in-time ring: feature tile by feature tile -- a fragment pair is refilled for the NEXT k-step as soon as its
                        // 3 JT MFMAs are issued (3 JT (IT - 1) MFMAs of cover), 8 IT registers of ring instead of 16 IT
#pragma unroll
                        for (int it = 0; it < IT; ++it) {
#pragma unroll
                            for (int jt = 0; jt < JT; ++jt) c[it][jt] = mf(ah[it], bh[cur][jt], c[it][jt]);
#pragma unroll
                            for (int jt = 0; jt < JT; ++jt) c[it][jt] = mf(ah[it], bl[cur][jt], c[it][jt]);
#pragma unroll
                            for (int jt = 0; jt < JT; ++jt) c[it][jt] = mf(al[it], bh[cur][jt], c[it][jt]);
                            if (LOADS) {
                                rh[0][it] = *reinterpret_cast<const h8 *>(base_h + pfo + (size_t)it * 1024);
                                rl[0][it] = *reinterpret_cast<const h8 *>(base_l + pfo + (size_t)it * 1024);
                            }
                        }
#pragma unroll
                        for (int it = 0; it < IT; ++it) {
                            if (it == 0) {
#pragma unroll
                                for (int i = 0; i < 2 * JT; ++i) {
                                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                                }
                                __builtin_amdgcn_sched_group_barrier(0x008, JT, 0);
                            } else {
                                __builtin_amdgcn_sched_group_barrier(0x008, 3 * JT, 0);
                            }
                            if (LOADS) __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
                        }
                    } else {
#pragma unroll
                    for (int it = 0; it < IT; ++it)
#pragma unroll
                        for (int jt = 0; jt < JT; ++jt) c[it][jt] = mf(ah[it], bh[cur][jt], c[it][jt]);
#pragma unroll
                    for (int it = 0; it < IT; ++it)
#pragma unroll
                        for (int jt = 0; jt < JT; ++jt) c[it][jt] = mf(ah[it], bl[cur][jt], c[it][jt]);
#pragma unroll
                    for (int it = 0; it < IT; ++it)
#pragma unroll
                        for (int jt = 0; jt < JT; ++jt) c[it][jt] = mf(al[it], bh[cur][jt], c[it][jt]);
                    if (LOADS) {
#pragma unroll
                        for (int it = 0; it < IT; ++it) {
                            rh[j][it] = *reinterpret_cast<const h8 *>(base_h + pfo + (size_t)(j * IT + it) * 1024);
                            rl[j][it] = *reinterpret_cast<const h8 *>(base_l + pfo + (size_t)(j * IT + it) * 1024);
                        }
                    }
                    // the product loop's pinned order, generalised: (M L) x 2JT, (n M, G) x 2IT, rest
                    constexpr int NM = 3 * IT * JT, NL = 2 * JT, NV = LOADS ? 2 * IT : 0;
#pragma unroll
                    for (int i = 0; i < NL; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    }
                    if constexpr (NV > 0) {
                        constexpr int PER = (NM - NL) / NV;
#pragma unroll
                        for (int i = 0; i < NV; ++i) {
                            __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);
                            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                        }
                        if constexpr (NM - NL - PER * NV > 0) __builtin_amdgcn_sched_group_barrier(0x008, NM - NL - PER * NV, 0);
                    } else {
                        __builtin_amdgcn_sched_group_barrier(0x008, NM - NL, 0);
                    }
                    }
                }
                bk += RING * 32;
                pf += RING;
                if (pf == NG * KS) pf = 0;
            }
        }
    };

    stamp(stamps, 0);
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll 1
        for (int g = 0; g < NG; g += 2) {
            if constexpr (CHECK) {
                gemm(acc[0]);
#pragma unroll
                for (int it = 0; it < IT; ++it)
#pragma unroll
                    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) chk[((size_t)tid * IT + it) * JT * 16 + jt * 16 + r] = acc[0][it][jt][r];
                return;
            }
            if constexpr (PARK) {  // the residual stream leaves for the scratch while fc_0 accumulates, and comes back for fc_1
                f32x4 *ws = park_ws + (size_t)blockIdx.x * (IT * JT * 4 * NWV * 64);
#pragma unroll
                for (int it = 0; it < IT; ++it)
#pragma unroll
                    for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const f32x4 v = {acc[0][it][jt][4 * k], acc[0][it][jt][4 * k + 1], acc[0][it][jt][4 * k + 2], acc[0][it][jt][4 * k + 3]};
                            ws[((it * JT + jt) * 4 + k) * (NWV * 64) + tid] = v;
                        }
            }
            gemm(acc[0]);
            if constexpr (PARK) {
                // the product's split epilogue consumes net here; one value per accumulator tile keeps the GEMM alive
#pragma unroll
                for (int it = 0; it < IT; ++it)
#pragma unroll
                    for (int jt = 0; jt < JT; ++jt) sink += acc[0][it][jt][(it + jt) & 15];
                const f32x4 *ws = park_ws + (size_t)blockIdx.x * (IT * JT * 4 * NWV * 64);
#pragma unroll
                for (int it = 0; it < IT; ++it)
#pragma unroll
                    for (int jt = 0; jt < JT; ++jt) {
                        __builtin_amdgcn_sched_barrier(0);  // one accumulator tile (4 loads) in flight at a time: no register spike
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            // (a rotated slot: the compiler cannot forward the stores; loads may target AGPRs directly)
                            const f32x4 v = ws[(((it * JT + jt) * 4 + k + 1) % (IT * JT * 4)) * (NWV * 64) + tid];
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[0][it][jt][4 * k + e] = v[e];
                        }
                    }
            }
            gemm(acc[NACC - 1]);
        }
    }
    stamp(stamps, 1);
    float s = sink;
#pragma unroll
    for (int a = 0; a < NACC; ++a)
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
            for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                for (int r = 0; r < 16; ++r) s += acc[a][it][jt][r];
    out[(size_t)blockIdx.x * (NWV * 64) + tid] = s;
}

// The shipped footprint on v_mfma_f32_16x16x32_f16.  Lane (c = l & 15, g = l >> 4); wave w owns 4 feature tiles t of 16 rows and the
// tile's 64 points as 4 point tiles jt of 16.  One stream step = one K = 32 step: per blob 4 tiles x 1 KiB, lane l's 16 bytes =
// A[row c][8 K values of group g]; the matching B fragment is the 16 bytes at K-step * 64 + 16 g of image row 16 jt + c.  Register
// r of accumulator (t, jt) is feature row 16 t + 4 g + r of point 16 jt + c.  The ring holds RING = 2 steps (16 KiB per wave, as
// shipped); a step's 8 fragments are refilled under the 12 MFMAs of its last point tile, once those have read them.
// B is fetched just in time: the (head, tail) pair of the NEXT point tile is read under the first two MFMAs of the current one.
template <int NACC, bool LOADS, bool CHECK = false>
__global__ void __launch_bounds__(512) gemm_ub16(const char *__restrict__ wstream, size_t tail_delta, float *__restrict__ out,
                                                 f32x4 *__restrict__, float *__restrict__ chk,
                                                 unsigned long long *__restrict__ stamps, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NWV = 8, NT = 4, NJ = 4, RING = 2, MT = 64, KS32 = D / 32;
    constexpr int ROW = D * 2 + 16;
    constexpr int LO_DELTA = MT * ROW;
    static_assert(KS32 % RING == 0 && (NG * KS32) % RING == 0 && (RING * NJ) % 2 == 0, "ring / B rotation parity");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    for (int i = tid; i < 2 * MT * ROW / 2; i += NWV * 64) reinterpret_cast<_Float16 *>(smem)[i] = image_value(i);
    __syncthreads();

    const size_t wave_bytes = (size_t)NG * KS32 * NT * 1024;
    const char *base_h = wstream + (size_t)wv * wave_bytes + lane * 16;
    const char *base_l = base_h + tail_delta;
    h8 rh[RING][NT], rl[RING][NT];
#pragma unroll
    for (int j = 0; j < RING; ++j)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            rh[j][t] = *reinterpret_cast<const h8 *>(base_h + (size_t)(j * NT + t) * 1024);
            rl[j][t] = *reinterpret_cast<const h8 *>(base_l + (size_t)(j * NT + t) * 1024);
        }
    int pf = RING;  // next K step (of NG * KS32) to prefetch
    ring_landed();

    f32x4 acc[NACC][NT][NJ];
#pragma unroll
    for (int a = 0; a < NACC; ++a)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[a][t][jt][r] = 0.f;

    const uint32_t b0 = c * ROW + g * 16;

    auto gemm = [&](f32x4 (&cc)[NT][NJ]) {
        __syncthreads();
        h8 bh[2], bl[2];
        bh[0] = *reinterpret_cast<const h8 *>(smem + b0);
        bl[0] = *reinterpret_cast<const h8 *>(smem + b0 + LO_DELTA);
        uint32_t bk = b0;
#pragma unroll 1
        for (int body = 0; body < KS32 / RING; ++body) {
            const size_t pfo = (size_t)pf * (NT * 1024);
#pragma unroll
            for (int j = 0; j < RING; ++j) {
#pragma unroll
                for (int jt = 0; jt < NJ; ++jt) {
                    const int cur = (j * NJ + jt) & 1;
                    const bool lastj = jt == NJ - 1;
                    const bool lastk = lastj && (j == RING - 1) && (body == KS32 / RING - 1);
                    // (after the last point tile of the last K step: step 0 again, read and dropped)
                    const uint32_t nx = lastk ? b0 : lastj ? bk + (j + 1) * 64 : bk + j * 64 + (jt + 1) * 16 * ROW;
                    bh[cur ^ 1] = *reinterpret_cast<const h8 *>(smem + nx);
                    bl[cur ^ 1] = *reinterpret_cast<const h8 *>(smem + nx + LO_DELTA);
#pragma unroll
                    for (int t = 0; t < NT; ++t) cc[t][jt] = mf16(rh[j][t], bh[cur], cc[t][jt]);
#pragma unroll
                    for (int t = 0; t < NT; ++t) cc[t][jt] = mf16(rh[j][t], bl[cur], cc[t][jt]);
#pragma unroll
                    for (int t = 0; t < NT; ++t) cc[t][jt] = mf16(rl[j][t], bh[cur], cc[t][jt]);
                    if (LOADS && lastj) {
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            rh[j][t] = *reinterpret_cast<const h8 *>(base_h + pfo + (size_t)(j * NT + t) * 1024);
                            rl[j][t] = *reinterpret_cast<const h8 *>(base_l + pfo + (size_t)(j * NT + t) * 1024);
                        }
                    }
                    // pinned order: (M L) x 2, then the rest of the 12 MFMAs; under the last point tile of a step the final
                    // pass (tail x head, the last reader of both fragments of a tile) carries the step's refill, 2 loads per MFMA
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    if (LOADS && lastj) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 2 * NT - 2, 0);
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                            __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
                        }
                    } else {
                        __builtin_amdgcn_sched_group_barrier(0x008, 3 * NT - 2, 0);
                    }
                }
            }
            bk += RING * 64;
            pf += RING;
            if (pf == NG * KS32) pf = 0;
        }
    };

    stamp(stamps, 0);
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
#pragma unroll 1
        for (int gg = 0; gg < NG; gg += 2) {
            if constexpr (CHECK) {
                gemm(acc[0]);
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) chk[((size_t)tid * NT + t) * NJ * 4 + jt * 4 + r] = acc[0][t][jt][r];
                return;
            }
            gemm(acc[0]);
            gemm(acc[NACC - 1]);
        }
    }
    stamp(stamps, 1);
    float s = 0.f;
#pragma unroll
    for (int a = 0; a < NACC; ++a)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
                for (int r = 0; r < 4; ++r) s += acc[a][t][jt][r];
    out[(size_t)blockIdx.x * (NWV * 64) + tid] = s;
}

using Kern = void (*)(const char *, size_t, float *, f32x4 *, float *, unsigned long long *, int);

struct Ctx {
    const char *d_w;
    size_t tail_delta;
    float *d_out;
    f32x4 *d_ws;
    float *d_chk;
    unsigned long long *d_stamps;
};

struct Form {
    const char *name;
    Kern kern;
    int threads, mt, tiles_per_wg;  // mt: points per tile
    size_t lds;
    int regs, scratch;
};

constexpr int NCU = 256;

static Form make_form(const char *name, Kern kern, int threads, int mt, int tiles_per_wg, size_t lds) {
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipFuncAttributes fa;
    CK(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(kern)));
    return Form{name, kern, threads, mt, tiles_per_wg, lds, fa.numRegs, (int)fa.localSizeBytes};
}

struct Clock { double ghz, mcycles; };  // in-kernel clock and shader cycles of one launch's tile loop, median over workgroups

// us per launch over `reps` back-to-back launches (after one warm-up launch)
static double time_form(const Form &f, const Ctx &c, int reps, Clock *clk = nullptr) {
    const int ntiles = NCU * f.tiles_per_wg;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    hipLaunchKernelGGL(f.kern, dim3(NCU), dim3(f.threads), f.lds, 0, c.d_w, c.tail_delta, c.d_out, c.d_ws, c.d_chk, c.d_stamps, ntiles);
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0));
    for (int i = 0; i < reps; ++i)
        hipLaunchKernelGGL(f.kern, dim3(NCU), dim3(f.threads), f.lds, 0, c.d_w, c.tail_delta, c.d_out, c.d_ws, c.d_chk, c.d_stamps, ntiles);
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    CK(hipGetLastError());
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
#ifdef UB_STAMP
    if (clk) {  // the last launch's stamps
        std::vector<unsigned long long> st((size_t)NCU * 4);
        CK(hipMemcpy(st.data(), c.d_stamps, st.size() * sizeof(st[0]), hipMemcpyDeviceToHost));
        std::vector<double> ghz, cyc;
        for (int b = 0; b < NCU; ++b) {
            const double dc = (double)(st[4 * b + 2] - st[4 * b]), dr = (double)(st[4 * b + 3] - st[4 * b + 1]);
            if (dr > 0) { ghz.push_back(dc / dr * 0.1); cyc.push_back(dc * 1e-6); }
        }
        std::sort(ghz.begin(), ghz.end());
        std::sort(cyc.begin(), cyc.end());
        clk->ghz = ghz.empty() ? 0 : ghz[ghz.size() / 2];
        clk->mcycles = cyc.empty() ? 0 : cyc[cyc.size() / 2];
    }
#else
    if (clk) *clk = Clock{0, 0};
#endif
    return ms * 1e3 / reps;
}

static double rate(const Form &f, double us) { return (double)NCU * f.tiles_per_wg * f.mt * NG / (us * 1e-6); }

template <int NWV, int IT, int JT, int RING, int NACC, bool KHALF, bool PARK, bool LOADS>
static Form wide_form(const char *name, int tiles_per_wg) {
    constexpr int KIMG = KHALF ? D / 2 : D;
    return make_form(name, gemm_ub<NWV, IT, JT, RING, NACC, KHALF, PARK, LOADS>, NWV * 64, JT * 32, tiles_per_wg,
                     2 * (size_t)(JT * 32) * (KIMG * 2 + 16));
}

template <int NWV, int IT, int JT, int RING, int NACC, bool KHALF, bool PARK, bool LOADS>
static double run(const char *name, const Ctx &c, int tiles_per_wg, int reps, double ref_rate) {
    const Form f = wide_form<NWV, IT, JT, RING, NACC, KHALF, PARK, LOADS>(name, tiles_per_wg);
    const double us = time_form(f, c, reps), r = rate(f, us);
    printf("%-34s waves %d IT %d JT %d ring %d acc-sets %d | regs %3d (spill/scratch %d B) LDS %6zu | %9.1f us | %7.2f G pt.gemm/s | %7.1f TF executed | x%.3f\n",
           name, NWV, IT, JT, RING, NACC, f.regs, f.scratch, f.lds, us, r / 1e9, r * (2.0 * D * D * 3) / 1e12, ref_rate > 0 ? r / ref_rate : 1.0);
    fflush(stdout);
    return r;
}

// ---- the on-device check of the fragment maps: ONE GEMM of one 64-point tile against the host -------------------------------
// The stream is arbitrary data, so "the weight matrix" is whatever the form's stream layout says it is: row `row` of feature tile
// `tile` of wave `wv`, K values k..k+7, are the 16 bytes of lane `lane_of(row, k)` in the 1 KiB fragment (step, tile).
struct Maps {
    int kstep;          // K per stream step (16 | 32)
    int tiles, rows;    // feature tiles per wave, rows per tile
    int jts, cols;      // point tiles, points per tile
    int nreg;           // accumulator registers per (tile, jt)
    int (*row_of)(int lane, int r);
    int (*col_of)(int lane);
};

static bool check_form(const char *name, Kern kern, size_t lds, const Maps &m, const std::vector<_Float16> &hw, size_t blob_elems,
                       const Ctx &c) {
    constexpr int ROW = D * 2 + 16, MT = 64;
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int per_thread = m.tiles * m.jts * m.nreg;
    CK(hipMemset(c.d_chk, 0xff, (size_t)512 * per_thread * sizeof(float)));
    hipLaunchKernelGGL(kern, dim3(1), dim3(512), lds, 0, c.d_w, c.tail_delta, c.d_out, c.d_ws, c.d_chk, c.d_stamps, 1);
    CK(hipDeviceSynchronize());
    CK(hipGetLastError());
    std::vector<float> got((size_t)512 * per_thread);
    CK(hipMemcpy(got.data(), c.d_chk, got.size() * sizeof(float), hipMemcpyDeviceToHost));
    // images as the kernel fills them, widened once
    std::vector<float> xh((size_t)MT * D), xl((size_t)MT * D);
    for (int p = 0; p < MT; ++p)
        for (int k = 0; k < D; ++k) {
            xh[(size_t)p * D + k] = (float)image_value(p * ROW / 2 + k);
            xl[(size_t)p * D + k] = (float)image_value((MT * ROW + p * ROW) / 2 + k);
        }
    const int steps = D / m.kstep, groups = m.kstep / 8;
    const size_t wave_elems = (size_t)NG * steps * m.tiles * 512;  // 1 KiB = 512 f16 per fragment
    double worst = 0;
    long bad = 0;
    for (int wv = 0; wv < 8; ++wv)
        for (int lane = 0; lane < 64; ++lane)
            for (int t = 0; t < m.tiles; ++t)
                for (int r = 0; r < m.nreg; ++r) {
                    const int row = m.row_of(lane, r);
                    for (int jt = 0; jt < m.jts; ++jt) {
                        const int p = jt * m.cols + m.col_of(lane);
                        double ref = 0, mag = 0;
                        for (int s = 0; s < steps; ++s)
                            for (int gq = 0; gq < groups; ++gq) {
                                const size_t a = (size_t)wv * wave_elems + ((size_t)s * m.tiles + t) * 512 + (size_t)(row + m.rows * gq) * 8;
                                for (int j = 0; j < 8; ++j) {
                                    const int k = s * m.kstep + gq * 8 + j;
                                    const double ah = (float)hw[a + j], al = (float)hw[blob_elems + a + j];
                                    const double bh = xh[(size_t)p * D + k], bl = xl[(size_t)p * D + k];
                                    ref += ah * bh + ah * bl + al * bh;
                                    mag += std::fabs(ah * bh) + std::fabs(ah * bl) + std::fabs(al * bh);
                                }
                            }
                        const float g = got[((size_t)(wv * 64 + lane) * m.tiles + t) * m.jts * m.nreg + jt * m.nreg + r];
                        const double err = std::fabs((double)g - ref) / (mag + 1e-30);
                        if (!(err <= 1e-5)) ++bad;  // fp32 accumulation of 1536 exact products: ~1e-7 of the magnitude; a wrong map: ~1
                        if (!(err <= worst)) worst = err;
                    }
                }
    printf("# check %-28s one GEMM, one 64-point tile, %d values vs host fp64: worst |err| / sum|terms| = %.2e, %ld bad -> %s\n", name,
           512 * per_thread, worst, bad, bad ? "FAILED" : "ok");
    fflush(stdout);
    return bad == 0;
}

static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}

int main(int argc, char **argv) {
    const bool wide = argc > 1 && !strcmp(argv[1], "--wide");
    const int a0 = wide ? 2 : 1;
    const int reps = argc > a0 ? atoi(argv[a0]) : (wide ? 5 : 100);
    const int rounds = argc > a0 + 1 ? atoi(argv[a0 + 1]) : 7;
    if (reps < 1 || rounds < 1) { fprintf(stderr, "usage: split_gemm [--wide] [reps [rounds]]\n"); return 2; }
    // one (head | tail) stream: NG x 512 x 512 x 2 B per blob -- 5.24 MB + 5.24 MB, the product's 10.8 MB footprint
    const size_t blob = (size_t)NG * D * D * 2;
    std::vector<_Float16> hw(blob);  // (elements: blob bytes = 2 blobs x blob/2 elements x 2 B)
    uint32_t s = 12345u;
    for (size_t i = 0; i < hw.size(); ++i) {
        s = s * 1664525u + 1013904223u;
        const float v = ((int)(s >> 9) % 2001 - 1000) * (i < blob / 2 ? 4.0e-5f : 2.0e-8f);  // heads ~ +-0.04, tails ~ +-2e-5
        hw[i] = (_Float16)v;
    }
    char *d_w;
    Ctx c;
    CK(hipMalloc(&d_w, 2 * blob));
    CK(hipMemcpy(d_w, hw.data(), 2 * blob, hipMemcpyHostToDevice));
    c.d_w = d_w;
    c.tail_delta = blob;
    CK(hipMalloc(&c.d_out, NCU * 512 * sizeof(float)));
    CK(hipMalloc(&c.d_ws, (size_t)NCU * 256 * 1024));  // 256 KiB per workgroup
    CK(hipMalloc(&c.d_chk, (size_t)512 * 64 * sizeof(float)));
    CK(hipMalloc(&c.d_stamps, (size_t)NCU * 4 * sizeof(unsigned long long)));
    CK(hipMemset(c.d_stamps, 0, (size_t)NCU * 4 * sizeof(unsigned long long)));
    hipDeviceProp_t pr;
    CK(hipGetDeviceProperties(&pr, 0));
    printf("# %s, %d CUs; %d GEMMs of 512 x 512 (head + tail = %.2f MB) per tile pass; persistent, one workgroup per CU\n", pr.gcnArchName,
           pr.multiProcessorCount, NG, 2 * blob / 1e6);
    if (wide) {
        // every form does the same number of (point, GEMM) products per workgroup: 768 points
        //                     NWV IT JT RING NACC KHALF  PARK   LOADS
        const double ref = run<8, 2, 2, 4, 2, false, false, true>("shipped (64 pt, 2 waves/SIMD)", c, 12, reps, 0);
        run<8, 2, 2, 4, 2, false, false, false>("shipped, ring never refilled", c, 12, reps, ref);
        run<4, 4, 2, 2, 2, false, false, true>("1 wave/SIMD, 64 pt (JT 2)", c, 12, reps, ref);
        run<4, 4, 3, 2, 2, true, false, true>("wide-96  (x + net live), ring 2", c, 8, reps, ref);
        run<4, 4, 3, 2, 1, true, false, true>("wide-96  (one acc set), ring 2", c, 8, reps, ref);
        run<4, 4, 3, 4, 1, true, false, true>("wide-96  (one acc set), ring 4", c, 8, reps, ref);
        run<4, 4, 4, 2, 1, true, false, true>("wide-128 (x parked: no traffic)", c, 6, reps, ref);
        run<4, 4, 3, 1, 2, true, false, true>("wide-96  (x + net live), JIT ring", c, 8, reps, ref);
        run<4, 4, 3, 1, 1, true, false, true>("wide-96  (one acc set), JIT ring", c, 8, reps, ref);
        run<4, 4, 3, 2, 1, true, true, true>("wide-96  + park round trips", c, 8, reps, ref);
        run<4, 4, 4, 2, 1, true, true, true>("wide-128 + park round trips", c, 6, reps, ref);
        run<4, 4, 4, 2, 1, true, false, false>("wide-128, ring never refilled", c, 6, reps, ref);
        // the shipped wave geometry (8 waves x 64 features: the packed stream's layout) with the residual stream parked: one
        // accumulator set of 32 JT registers per feature tile, K-half-staged images
        run<8, 2, 3, 4, 1, true, false, true>("8 waves, 96 pt, K halves", c, 8, reps, ref);
        run<8, 2, 3, 4, 1, true, true, true>("8 waves, 96 pt, K halves + park", c, 8, reps, ref);
        run<8, 2, 3, 2, 1, true, true, true>("8 waves, 96 pt + park, ring 2", c, 8, reps, ref);
        run<8, 2, 4, 2, 1, true, true, true>("8 waves, 128 pt + park, ring 2", c, 6, reps, ref);
        run<8, 2, 4, 4, 1, true, true, true>("8 waves, 128 pt + park, ring 4", c, 6, reps, ref);
        run<8, 2, 2, 4, 1, false, true, true>("8 waves, 64 pt + park (x1 check)", c, 12, reps, ref);
        return 0;
    }

    // ---- the shape gate -------------------------------------------------------------------------------------------------------
    const size_t lds64 = 2 * (size_t)64 * (D * 2 + 16);
    const Maps m32{16, 2, 32, 2, 32, 16, [](int l, int r) { return (r & 3) + 8 * (r >> 2) + 4 * (l >> 5); }, [](int l) { return l & 31; }};
    const Maps m16{32, 4, 16, 4, 16, 4, [](int l, int r) { return 4 * (l >> 4) + r; }, [](int l) { return l & 15; }};
    bool ok = check_form("shipped (32x32x16)", gemm_ub<8, 2, 2, 4, 2, false, false, true, true>, lds64, m32, hw, blob / 2, c);
    ok = check_form("16x16x32", gemm_ub16<2, true, true>, lds64, m16, hw, blob / 2, c) && ok;
    if (!ok) { fprintf(stderr, "fragment-map check failed: nothing timed\n"); return 1; }

    // "shipped" is in the rotation twice: the second copy against the first is the spread of shipped against itself
    const Form forms[] = {
        make_form("shipped 32x32x16", gemm_ub<8, 2, 2, 4, 2, false, false, true>, 512, 64, 12, lds64),
        make_form("16x16x32", gemm_ub16<2, true>, 512, 64, 12, lds64),
        make_form("shipped 32x32x16 (again)", gemm_ub<8, 2, 2, 4, 2, false, false, true>, 512, 64, 12, lds64),
        make_form("shipped, ring never refilled", gemm_ub<8, 2, 2, 4, 2, false, false, false>, 512, 64, 12, lds64),
        make_form("16x16x32, ring never refilled", gemm_ub16<2, false>, 512, 64, 12, lds64),
    };
    constexpr int NF = sizeof(forms) / sizeof(forms[0]);
    std::vector<double> us[NF];
    Clock clk[NF];
    printf("# %d rounds, forms interleaved in one process, %d back-to-back launches per sample; us per launch:\n# round", rounds, reps);
    for (int f = 0; f < NF; ++f) printf(" | %s", forms[f].name);
    printf("\n");
    for (int f = 0; f < NF; ++f) time_form(forms[f], c, reps);  // one unrecorded pass: code objects loaded, clocks settled
    for (int r = 0; r < rounds; ++r) {
        printf("  %5d", r);
        for (int f = 0; f < NF; ++f) {
            us[f].push_back(time_form(forms[f], c, reps, &clk[f]));
            printf(" | %9.1f", us[f].back());
        }
        printf("\n");
        fflush(stdout);
    }
    const double ref_med = median(us[0]), ref_min = *std::min_element(us[0].begin(), us[0].end());
    for (int f = 0; f < NF; ++f) {
        const double med = median(us[f]), mn = *std::min_element(us[f].begin(), us[f].end()), mx = *std::max_element(us[f].begin(), us[f].end());
        double lo = 1e30, hi = 0;  // per-round rate ratio to shipped
        for (int r = 0; r < rounds; ++r) { lo = std::min(lo, us[0][r] / us[f][r]); hi = std::max(hi, us[0][r] / us[f][r]); }
        printf("%-30s regs %3d (scratch %d B) | median %9.1f us  min %9.1f  max %9.1f | %7.1f TF executed (median) | rate vs shipped: median x%.4f  min x%.4f"
               "  per round x%.4f .. x%.4f",
               forms[f].name, forms[f].regs, forms[f].scratch, med, mn, mx, rate(forms[f], med) * (2.0 * D * D * 3) / 1e12, ref_med / med,
               ref_min / mn, lo, hi);
#ifdef UB_STAMP
        printf(" | in-kernel clock %.3f GHz, %.2f Mcycles per launch (last round)", clk[f].ghz, clk[f].mcycles);
#endif
        printf("\n");
    }
    {
        double lo = 1e30, hi = 0;
        for (int r = 0; r < rounds; ++r) { lo = std::min(lo, us[0][r] / us[2][r]); hi = std::max(hi, us[0][r] / us[2][r]); }
        const double spread = std::max(hi - 1.0, 1.0 - lo);
        double glo = 1e30;
        for (int r = 0; r < rounds; ++r) glo = std::min(glo, us[0][r] / us[1][r]);
        printf("# spread of shipped against itself (same round, worst of %d): %.2f %%;  16x16x32 vs shipped, worst round: %+.2f %%, median of medians: %+.2f %%\n",
               rounds, 100 * spread, 100 * (glo - 1.0), 100 * (ref_med / median(us[1]) - 1.0));
        printf("# gate (16x16x32 faster than shipped by wall, in every round, by more than that spread): %s\n",
               glo - 1.0 > spread ? "PASSED" : "NOT passed");
    }
    return 0;
}
