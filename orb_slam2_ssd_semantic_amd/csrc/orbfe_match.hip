// orbfe_match.hip -- Hamming matcher kernels + C-ABI (include/orbfe.h "Matcher").
//
// Reference behaviour restated (paths relative to /root/reference):
//   DescriptorDistance                 src/ORBmatcher.cc:1968-1984
//   best / second-best update idiom    src/ORBmatcher.cc:280-289 (and :732-741)
//   SearchByBoW (KF,F) / (KF,KF)       src/ORBmatcher.cc:217-363 / :665-812
//   rotation histogram + prune         src/ORBmatcher.cc:308-316, :338-360
//   ComputeThreeMaxima                 src/ORBmatcher.cc:1912-1957
// Candidate-list matchers (SearchByBoW, CSR Hamming, stereo, BoW descent, distinctive descriptors): xor + v_bcnt_u32_b32.
// All-pairs brute force (M3): by default an EXACT FP4 dot product on the matrix cores (k_match_bf); the xor / popcount
// all-pairs kernel the north star names is kept as k_match_popc (orbfe_matcher_set_bf_kernel), bit-identical, slower
// (profiles/r02_match_variants.json).  No CPU path.
#include <stddef.h>
#include <algorithm>
#include <new>

#include <vector>

#include "orbfe_common.h"
#include "orbfe_kernels.h"
#include "orbfe_matcher.h"
#include "orbfe_match_dev.h"

// ---------------------------------------------------------------------------------------------------
// K8  brute force on the matrix cores.
//
// All-pairs Hamming is a GEMM in disguise: with every descriptor bit b mapped to 2b-1 on both sides,
//     dot(t', q') = 256 - 2 * hamming(q, t).
// +-1 needs one bit of operand, and the narrowest operand the matrix cores take is FP4 (E2M1), which holds +-1 exactly:
// v_mfma_scale_f32_32x32x64_f8f6f4 with FP4 on both sides evaluates a 32 x 32 tile of such dots over 64 bit positions per
// instruction, 4 of them cover the 256 bits, and the E8M0 block scales (2^5 on the train side, 1 on the query side; powers
// of two, exact) multiply the dot by 32.  Every partial sum is an integer below 2^17, exact in the fp32 accumulator.
// The accumulators do not start at zero but at (32 - train row inside the tile) + an offset, so that the fp32 BIT PATTERN
// of an accumulator IS the ranking key (orbfe_match_dev.h, bm_key_*; pinned by a static_assert over every distance and row)
//     bits = 0x47000000 + ((64 * (256 - d) + field) << 8)              (larger = closer, earlier row wins ties)
// and all that is left for the VALU is to keep, per query, the two largest keys as integers: 2.5 instructions per distance
// instead of the 20 of an xor/popcount loop, and no convert.  The best key gives (distance, lowest index) and the second key
// the second-smallest distance with multiplicity, which is exactly what the reference's sequential
//     if (d < best) {second = best; best = d; idx = j;} else if (d < second) second = d;
// produces.  Between train tiles the field of the running keys is forced to 63 (an older row beats any newer
// one on equal distance) and the global index of the best is latched whenever the best key changed in a tile.
//
// Workgroup = 4 waves x BM_Q query tiles of 32 (BM_Q = 4: 512 queries); the train descriptors stream through LDS in tiles of
// 32 rows (4 KB per buffer), expanded bit -> nibble on the way in (one table dword per source byte, one ds_write_b128 per
// source dword) and laid out so that the A operand of lane (row r, k-half h) at k-step s is one conflict-free ds_read_b128 at
// ((2s + h) * 32 + r) * 16.  The query tiles (B operands, 16 VGPRs each) are expanded once through the same table and stay in
// registers.  Lane (r, h) holds source dword 4h + s of its row at k-step s on both sides, nibble for nibble in the same
// order, and every block scale of a side is the same number, so whatever k the hardware gives an operand position, the dot
// product pairs bit i with bit i.
// The wave is software-pipelined: the MFMA chain of the next query tile (at the end of a train tile: of query tile 0
// of the next train tile) is issued between the ranking instructions of the current one.
// BM_Q is a template parameter, instantiated for 4 (the default of every caller), 2 and 1 under the same launch bound; the
// register counts (174, 133, 87) are in DESIGN.md sections 4 and 6.  A workgroup needs its registers on all four SIMDs of one CU at
// once; beside the dense FAST pass (three resident workgroups of 160 registers per SIMD) the 4-tile form fits where one of them
// has left (174 + 2 x 160 <= 512).  Fewer tiles re-read every train tile from the LDS more often per MFMA; the results are the
// same bytes.
// ---------------------------------------------------------------------------------------------------
#define BM_WAVES 4
#define BM_QUERIES(Q) (BM_WAVES * (Q) * 32)   // queries of a workgroup of Q tiles per wave
#define BM_MAX_NT (1 << 22)  // the index is latched as a plain int; only nt * 32 bytes must be addressable in 32 bits

typedef int bm_v4i __attribute__((ext_vector_type(4)));
typedef int bm_v16i __attribute__((ext_vector_type(16)));
typedef float bm_v16f __attribute__((ext_vector_type(16)));

// bit b of v -> nibble b: FP4 +1 if set, -1 if clear (one dword for the 8 bits)
__device__ __forceinline__ uint32_t bm_expand_byte(uint32_t v)
{
    uint32_t e = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) e |= (((v >> b) & 1u) ? BM_FP4_POS : BM_FP4_NEG) << (4 * b);
    return e;
}

// one k-step of the chain: 64 bit positions, FP4 x FP4 (cbsz 4, blgp 4: the low 4 registers of each operand are read)
__device__ __forceinline__ bm_v16f bm_mfma_fp4(const bm_v4i &a, const bm_v4i &b, const bm_v16f &acc)
{
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(__builtin_shufflevector(a, a, 0, 1, 2, 3, -1, -1, -1, -1),
                                                           __builtin_shufflevector(b, b, 0, 1, 2, 3, -1, -1, -1, -1), acc, 4, 4, 0,
                                                           (int)BM_SCALE_TRAIN, 0, (int)BM_SCALE_QUERY);
}

template <int BM_Q>
__global__ __launch_bounds__(BM_WAVES * 64, 2) void k_match_bf(const uint8_t *__restrict__ q_base,
                                                               const uint8_t *__restrict__ t_base,
                                                               const int32_t *__restrict__ n_arr,  // per-frame counts or NULL
                                                               const int32_t *__restrict__ tn_arr, // counts of the train block
                                                               const int32_t *__restrict__ qframe,
                                                               const int32_t *__restrict__ tframe, int cap, int nq_s,
                                                               int nt_s, float nnratio, int th,
                                                               int32_t *__restrict__ match, int32_t *__restrict__ best_o,
                                                               int32_t *__restrict__ second_o)
{
    __shared__ uint32_t s_tab[256];  // source byte -> 8 FP4 nibbles of +-1 (both sides)
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[2][32 * 128];
    const int pair = blockIdx.y;
    const uint8_t *q = q_base, *t = t_base;
    int nq = nq_s, nt = nt_s;
    int64_t out0 = 0;
    if (n_arr) {  // batched-frames form
        const int qf = qframe[pair], tf = tframe[pair];
        q = q_base + (int64_t)qf * cap * 32;
        t = t_base + (int64_t)tf * cap * 32;
        nq = min(n_arr[qf], cap);
        nt = min(tn_arr[tf], cap);
        out0 = (int64_t)pair * cap;
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int BM_QW = BM_QUERIES(BM_Q);
    const int q0 = blockIdx.x * BM_QW;
    const int nslots = n_arr ? cap : nq;  // output slots of this pair
    if (q0 >= nslots) return;
    if (q0 >= nq) {  // only padding slots of the batched form: no match, no compute
        for (int i = q0 + tid; i < min(q0 + BM_QW, nslots); i += BM_WAVES * 64) {
            match[out0 + i] = -1;
            if (best_o) best_o[out0 + i] = 256;
            if (second_o) second_o[out0 + i] = 256;
        }
        return;
    }
    s_tab[tid] = bm_expand_byte((uint32_t)tid);
    __syncthreads();

    const int c = lane & 31, h = lane >> 5;
    // ---- B operands: BM_Q query tiles, lane (c, h) holds bits [128h, 128h + 128) of query c as 4 x 16 bytes ----
    bm_v4i B[BM_Q][4];
#pragma unroll
    for (int u = 0; u < BM_Q; ++u) {
        const int qi = q0 + (wid * BM_Q + u) * 32 + c;
        const uint4 raw = *(const uint4 *)(q + (int64_t)min(qi, nq - 1) * 32 + h * 16);
        const uint32_t rw[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int sstep = 0; sstep < 4; ++sstep)
            B[u][sstep] = bm_v4i{(int)s_tab[rw[sstep] & 0xFFu], (int)s_tab[(rw[sstep] >> 8) & 0xFFu],
                                 (int)s_tab[(rw[sstep] >> 16) & 0xFFu], (int)s_tab[rw[sstep] >> 24]};
    }
    int kb[BM_Q], ks[BM_Q], bi[BM_Q];
#pragma unroll
    for (int u = 0; u < BM_Q; ++u) {
        kb[u] = ks[u] = BM_KEY_NONE;
        bi[u] = -1;
    }
    if (nt > 0) {
        // ---- train tile staging: thread (r = tid & 31, w = tid >> 5) expands source dword w of row r ----
        const int sr = tid & 31, sw = tid >> 5;
        const uint32_t *t32 = (const uint32_t *)t;
        // rows past the end re-read the last row: their keys are masked in the last tile
        auto stage_load = [&](int T) -> uint32_t { return t32[(uint32_t)(min(T + sr, nt - 1) * 8 + sw)]; };
        // source dword sw = 4 hh + s of row sr is the 16 bytes lane (sr, hh) reads at k-step s
        auto stage_store = [&](uint32_t dw, int buf) {
            const int off = (((sw & 3) * 2 + (sw >> 2)) * 32 + sr) * 16;
            *(uint4 *)(s_tile[buf] + off) = make_uint4(s_tab[dw & 0xFFu], s_tab[(dw >> 8) & 0xFFu], s_tab[(dw >> 16) & 0xFFu], s_tab[dw >> 24]);
        };
        auto load_a = [&](bm_v4i (&A)[4], int buf) {
#pragma unroll
            for (int sstep = 0; sstep < 4; ++sstep)
                A[sstep] = *(const bm_v4i *)(s_tile[buf] + ((sstep * 2 + h) * 32 + c) * 16);
        };
        // accumulator start values: the key of (no agreeing bit yet, train row of the accumulator inside the tile)
        bm_v16f cfull;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) cfull[reg] = bm_key_start((reg & 3) + 8 * (reg >> 2) + 4 * h);
        auto chain = [&](const bm_v4i (&A)[4], const bm_v4i (&Bu)[4]) -> bm_v16i {
            bm_v16f acc = cfull;
#pragma unroll
            for (int sstep = 0; sstep < 4; ++sstep) acc = bm_mfma_fp4(A[sstep], Bu[sstep], acc);
            return __builtin_bit_cast(bm_v16i, acc);  // the fp32 patterns are the keys
        };
        auto interleave = [&]() {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // one MFMA
                __builtin_amdgcn_sched_group_barrier(0x002, 13, 0);  // a quarter of the ranking VALU
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        // two largest keys of query tile u over the 16 rows in `acc`; latch the index when the best changed.
        // A tournament instead of a running (best, second) pair: same instruction count, but depth 5 instead of 16 --
        // with two waves per SIMD a 16-long dependent chain leaves the VALU idle most of the time.
        auto rank = [&](const bm_v16i &acc, int u, int T, bool mask_tail) {
            int hi[8], lo[8];
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                int k0 = acc[2 * p], k1 = acc[2 * p + 1];
                if (mask_tail) {
                    if (T + ((2 * p) & 3) + 8 * ((2 * p) >> 2) + 4 * h >= nt) k0 = BM_KEY_NONE;
                    if (T + ((2 * p + 1) & 3) + 8 * ((2 * p + 1) >> 2) + 4 * h >= nt) k1 = BM_KEY_NONE;
                }
                hi[p] = max(k0, k1);
                lo[p] = min(k0, k1);
            }
#pragma unroll
            for (int w = 4; w >= 1; w >>= 1)
#pragma unroll
                for (int p = 0; p < w; ++p) {  // merge the (largest, second) pairs p and p + w
                    const int h2 = max(hi[p], hi[p + w]);
                    lo[p] = max(min(hi[p], hi[p + w]), max(lo[p], lo[p + w]));
                    hi[p] = h2;
                }
            const int bprev = kb[u] | BM_KEY_FORCE, sprev = ks[u] | BM_KEY_FORCE;
            const int b = max(bprev, hi[0]);
            const int s2 = max(min(bprev, hi[0]), max(sprev, lo[0]));
            if (b != bprev) bi[u] = T + bm_key_row(b);
            kb[u] = b;
            ks[u] = s2;
        };

        stage_store(stage_load(0), 0);
        uint32_t g1 = stage_load(32);  // source dword of the tile after next, fetched two tiles before it is consumed
        __syncthreads();
        bm_v4i A[4];
        load_a(A, 0);
        bm_v16i acc = chain(A, B[0]);
        int buf = 0, T = 0;
        for (; T + 32 < nt; T += 32) {  // all tiles but the last one
            const uint32_t g2 = stage_load(T + 64);
            stage_store(g1, buf ^ 1);  // tile T + 32 (not read before the barrier below)
            g1 = g2;
#pragma unroll
            for (int u = 0; u < BM_Q; ++u) {
                bm_v16i nacc;
                if (u + 1 < BM_Q) {
                    nacc = chain(A, B[u + 1]);
                } else {  // next train tile
                    __syncthreads();
                    buf ^= 1;
                    load_a(A, buf);
                    nacc = chain(A, B[0]);
                }
                rank(acc, u, T, false);
                interleave();
                acc = nacc;
            }
        }
#pragma unroll
        for (int u = 0; u < BM_Q; ++u) {  // last tile: rows past the end of the train set are masked
            bm_v16i nacc = acc;
            if (u + 1 < BM_Q) nacc = chain(A, B[u + 1]);
            rank(acc, u, T, true);
            acc = nacc;
        }
    }
    // ---- lanes c and c + 32 hold different train rows of the same query: merge the two halves, decode ----
#pragma unroll
    for (int u = 0; u < BM_Q; ++u) {
        const int ob = __shfl_xor(kb[u], 32, 64), os = __shfl_xor(ks[u], 32, 64), oi = __shfl_xor(bi[u], 32, 64);
        // distance part of a key: larger = closer, 0 where no key was seen
        const int mb = bm_key_m(kb[u]), mo = bm_key_m(ob);
        const bool take_o = mo > mb || (mo == mb && oi >= 0 && (bi[u] < 0 || oi < bi[u]));
        const int m1 = take_o ? mo : mb, idx = take_o ? oi : bi[u];
        const int m2 = max(min(mb, mo), max(bm_key_m(ks[u]), bm_key_m(os)));
        const int qi = q0 + (wid * BM_Q + u) * 32 + c;
        if (h == 0 && qi < nslots) {
            const int best = idx >= 0 ? bm_m_dist(m1) : 256;
            const int second = m2 > 0 ? bm_m_dist(m2) : 256;
            const bool valid = qi < nq;
            int m = -1;
            // best < 256: with the reference's initial bestDist = 256 a row at distance 256 never becomes the best
            if (valid && idx >= 0 && best < 256 && best <= th && (float)best < __fmul_rn(nnratio, (float)second)) m = idx;
            match[out0 + qi] = m;
            if (best_o) best_o[out0 + qi] = valid ? best : 256;
            if (second_o) second_o[out0 + qi] = valid ? second : 256;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// K8b  brute force by xor / popcount (the all-pairs formulation BASELINE.json's north star names; kept for the A/B).
// One lane per query (descriptor in 8 VGPRs), the train rows stream through LDS in tiles of 128 and are read as
// broadcasts; per distance 8 v_xor + 8 v_bcnt_u32_b32 (accumulating) + 4 ranking ops on the unique key
// (distance << 22 | train index): b2 = min(b2, max(b1, k)); b1 = min(b1, k) keeps the two smallest keys, i.e. best
// distance with the lowest index and the second-smallest distance with multiplicity -- the reference's update idiom.
// Same arguments, same outputs as k_match_bf.
// ---------------------------------------------------------------------------------------------------
#define BP_TILE 128
__global__ __launch_bounds__(256) void k_match_popc(const uint8_t *__restrict__ q_base, const uint8_t *__restrict__ t_base,
                                                    const int32_t *__restrict__ n_arr, const int32_t *__restrict__ tn_arr,
                                                    const int32_t *__restrict__ qframe,
                                                    const int32_t *__restrict__ tframe, int cap, int nq_s, int nt_s,
                                                    float nnratio, int th, int32_t *__restrict__ match,
                                                    int32_t *__restrict__ best_o, int32_t *__restrict__ second_o)
{
    __shared__ uint4 s_t[BP_TILE][2];
    const int pair = blockIdx.y;
    const uint8_t *q = q_base, *t = t_base;
    int nq = nq_s, nt = nt_s;
    int64_t out0 = 0;
    if (n_arr) {
        const int qf = qframe[pair], tf = tframe[pair];
        q = q_base + (int64_t)qf * cap * 32;
        t = t_base + (int64_t)tf * cap * 32;
        nq = min(n_arr[qf], cap);
        nt = min(tn_arr[tf], cap);
        out0 = (int64_t)pair * cap;
    }
    const int tid = threadIdx.x;
    const int qi = blockIdx.x * 256 + tid;
    const int nslots = n_arr ? cap : nq;
    if ((int)blockIdx.x * 256 >= nslots) return;
    uint32_t qw[8];
    {
        const uint4 *pq = (const uint4 *)(q + (int64_t)min(qi, max(nq - 1, 0)) * 32);
        const uint4 a = nq > 0 ? pq[0] : make_uint4(0, 0, 0, 0), b = nq > 0 ? pq[1] : make_uint4(0, 0, 0, 0);
        qw[0] = a.x; qw[1] = a.y; qw[2] = a.z; qw[3] = a.w; qw[4] = b.x; qw[5] = b.y; qw[6] = b.z; qw[7] = b.w;
    }
    uint32_t k1 = 0xFFFFFFFFu, k2 = 0xFFFFFFFFu;
    for (int T = 0; T < nt; T += BP_TILE) {
        __syncthreads();
        {
            const int r = tid >> 1, hf = tid & 1;   // 256 threads stage 128 rows x 2 halves
            s_t[r][hf] = ((const uint4 *)(t + (int64_t)min(T + r, nt - 1) * 32))[hf];
        }
        __syncthreads();
        const int rows = min(BP_TILE, nt - T);
        for (int r = 0; r < rows; ++r) {
            const uint4 a = s_t[r][0], b = s_t[r][1];
            uint32_t d = __popc(qw[0] ^ a.x);
            d += __popc(qw[1] ^ a.y);
            d += __popc(qw[2] ^ a.z);
            d += __popc(qw[3] ^ a.w);
            d += __popc(qw[4] ^ b.x);
            d += __popc(qw[5] ^ b.y);
            d += __popc(qw[6] ^ b.z);
            d += __popc(qw[7] ^ b.w);
            const uint32_t k = (d << 22) | (uint32_t)(T + r);
            k2 = min(k2, max(k1, k));
            k1 = min(k1, k);
        }
    }
    if (qi < nslots) {
        const bool valid = qi < nq;
        const int best = k1 != 0xFFFFFFFFu ? (int)(k1 >> 22) : 256;
        const int second = k2 != 0xFFFFFFFFu ? (int)(k2 >> 22) : 256;
        const int idx = k1 != 0xFFFFFFFFu ? (int)(k1 & 0x3FFFFFu) : -1;
        int m = -1;
        if (valid && idx >= 0 && best < 256 && best <= th && (float)best < __fmul_rn(nnratio, (float)second)) m = idx;  // as k_match_bf
        match[out0 + qi] = m;
        if (best_o) best_o[out0 + qi] = valid ? best : 256;
        if (second_o) second_o[out0 + qi] = valid ? second : 256;
    }
}

// ---------------------------------------------------------------------------------------------------
// K10  rotation-consistency histogram over accepted matches, ComputeThreeMaxima, prune, count (rot_prune, orbfe_match_dev.h).
// One workgroup per pair.  key i is kept when its bin is one of the three maxima.
// angles: element i of side X is at X_ang[i * stride] (stride 1 for plain arrays, 7 for orbfe_keypoint).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rot_prune(int32_t *__restrict__ match, const float *__restrict__ a_ang,
                                                   const float *__restrict__ b_ang, int ang_stride,
                                                   const int32_t *__restrict__ n_arr,
                                                   const int32_t *__restrict__ aframe,
                                                   const int32_t *__restrict__ bframe, int cap, int n_s,
                                                   int check_ori, int32_t *__restrict__ nmatches)
{
    const int pair = blockIdx.x;
    int n = n_s;
    int32_t *mt = match;
    const float *aa = a_ang, *ba = b_ang;
    if (n_arr) {
        const int af = aframe[pair], bf = bframe[pair];
        n = min(n_arr[af], cap);
        mt = match + (int64_t)pair * cap;
        aa = a_ang + (int64_t)af * cap * ang_stride;
        ba = b_ang + (int64_t)bf * cap * ang_stride;
    }
    rot_prune(mt, n, check_ori, nmatches + pair, [&](int i, int) { return aa[(int64_t)i * ang_stride]; },
              [&](int, int j) { return ba[(int64_t)j * ang_stride]; });
}

// 8(f).1: best / second-best over a per-query candidate list
__global__ __launch_bounds__(256) void k_hamming_csr(const uint8_t *__restrict__ q, int nq,
                                                     const uint8_t *__restrict__ t, const uint32_t *__restrict__ off,
                                                     const uint32_t *__restrict__ cand, int32_t *__restrict__ best_idx,
                                                     int32_t *__restrict__ best, int32_t *__restrict__ second,
                                                     int32_t *__restrict__ second_idx)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    Desc8 dq;   // not load_desc8: through it this kernel compiles to other code (profiles/search_helpers_shared.md)
    const uint32_t *p = (const uint32_t *)(q + (int64_t)i * 32);
#pragma unroll
    for (int k = 0; k < 8; ++k) dq.w[k] = p[k];
    // the reference's update idiom (:128-140) with the bookkeeping it attaches to the runner-up (bestLevel2 = the level of
    // whichever candidate last set bestDist2): si = that candidate
    int b1 = 256, b2 = 256, bi = -1, si = -1;
    for (uint32_t j = off[i]; j < off[i + 1]; ++j) {
        const uint32_t c = cand[j];
        const int d = hamming8(dq, (const uint32_t *)(t + (int64_t)c * 32));
        if (d < b1) { b2 = b1; si = bi; b1 = d; bi = (int)c; }
        else if (d < b2) { b2 = d; si = (int)c; }
    }
    best_idx[i] = bi;
    best[i] = b1;
    second[i] = b2;
    if (second_idx) second_idx[i] = si;
}

// every distance of a candidate list, for callers whose acceptance rule needs more than the two smallest
// (SearchForInitialization, src/ORBmatcher.cc:571-574: a candidate is skipped when an earlier query already holds it at a
// smaller distance).  One wave per query, lanes over its candidates.
__global__ __launch_bounds__(256) void k_hamming_csr_all(const uint8_t *__restrict__ q, int nq, const uint8_t *__restrict__ t,
                                                         const uint32_t *__restrict__ off, const uint32_t *__restrict__ cand,
                                                         uint16_t *__restrict__ dist)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nq) return;
    const int lane = threadIdx.x & 63;
    const Desc8 dq = load_desc8(q + (int64_t)i * 32);
    const uint32_t e = off[i + 1];
    for (uint32_t j = off[i] + (uint32_t)lane; j < e; j += 64u)
        dist[j] = (uint16_t)hamming8(dq, (const uint32_t *)(t + (int64_t)cand[j] * 32));
}

// ---------------------------------------------------------------------------------------------------
// host API
// ---------------------------------------------------------------------------------------------------
extern "C" int32_t orbfe_hamming(const uint8_t a[32], const uint8_t b[32])
{
    // src/ORBmatcher.cc:1968-1984 (the SWAR popcount there equals a hardware popcount)
    int d = 0;
    for (int i = 0; i < 8; ++i) {
        uint32_t x, y;
        memcpy(&x, a + 4 * i, 4);
        memcpy(&y, b + 4 * i, 4);
        d += __builtin_popcount(x ^ y);
    }
    return d;
}

static orbfe_status matcher_create_impl(int32_t device, hipStream_t borrowed, bool borrow, orbfe_matcher **out);
extern "C" orbfe_status orbfe_matcher_create(int32_t device, orbfe_matcher **out) { return matcher_create_impl(device, nullptr, false, out); }
// a matcher for a pipe of orbfe_pipeline: `st` (the pipe's stream) is its own stream and stays the pipeline's
orbfe_status orbfe_internal_matcher_create_on_stream(int32_t device, void *st, orbfe_matcher **out)
{
    return matcher_create_impl(device, (hipStream_t)st, true, out);
}

static orbfe_status matcher_create_impl(int32_t device, hipStream_t borrowed, bool borrow, orbfe_matcher **out)
{
    if (!out) return ORBFE_ERR_ARG;
    *out = nullptr;
    const orbfe_status rs = orb_resolve_device(&device);
    if (rs != ORBFE_OK) return rs;
    orbfe_matcher *m = new (std::nothrow) orbfe_matcher();
    if (!m) return ORBFE_ERR_NOMEM;
    m->device = device;
    DeviceGuard g(device);
    m->own_stream = !borrow;
    if (borrow) m->stream = borrowed;
    if ((!borrow && hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) ||
        hipEventCreateWithFlags(&m->ev_scratch, hipEventDisableTiming) != hipSuccess) {
        orbfe_set_error("hipStreamCreate / hipEventCreate failed");
        if (m->stream && m->own_stream) (void)hipStreamDestroy(m->stream);
        delete m;
        return ORBFE_ERR_HIP;
    }
    *out = m;
    return ORBFE_OK;
}

extern "C" void *orbfe_matcher_get_stream(orbfe_matcher *m) { return m ? (void *)m->stream : nullptr; }

extern "C" orbfe_status orbfe_matcher_set_bf_kernel(orbfe_matcher *m, int32_t kernel)
{
    if (!m || kernel < 0 || kernel > 1) return ORBFE_ERR_ARG;
    m->bf_kernel = kernel;
    return ORBFE_OK;
}

// query tiles per wave of k_match_bf for this handle's brute-force calls: 4 (the default), 2 or 1.  Same results, fewer registers
// (not in include/orbfe.h: an A/B and test knob)
extern "C" orbfe_status orbfe_internal_matcher_set_bf_tiles(orbfe_matcher *m, int32_t tiles)
{
    if (!m || !orb_match_tiles_ok(tiles)) return ORBFE_ERR_ARG;
    m->bf_tiles = tiles;
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_matcher_set_projection_kernel(orbfe_matcher *m, int32_t kernel)
{
    if (!m || kernel < 0 || kernel > 1) return ORBFE_ERR_ARG;
    m->proj_fused = kernel == 0;
    return ORBFE_OK;
}

extern "C" void orbfe_matcher_destroy(orbfe_matcher *m)
{
    if (!m) return;
    DeviceGuard g(m->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    if (m->scratch_used) (void)hipEventSynchronize(m->ev_scratch);
    for (auto &b : m->b) b.release();
    m->proj_done.release();
    m->pin_in.release();
    m->pin_out.release();
    if (m->ev_scratch) (void)hipEventDestroy(m->ev_scratch);
    if (m->stream && m->own_stream) (void)hipStreamDestroy(m->stream);
    delete m;
}

// one launch of k_match_bf<tiles> (tiles 4, 2 or 1; the setters let nothing else through)
template <typename... Args>
static void launch_match_bf(int tiles, int nslots, int npairs, hipStream_t st, Args... args)
{
    const dim3 block(BM_WAVES * 64);
    auto grid = [&](int qw) { return dim3((nslots + qw - 1) / qw, npairs); };
    if (tiles == 1) hipLaunchKernelGGL(k_match_bf<1>, grid(BM_QUERIES(1)), block, 0, st, args...);
    else if (tiles == 2) hipLaunchKernelGGL(k_match_bf<2>, grid(BM_QUERIES(2)), block, 0, st, args...);
    else hipLaunchKernelGGL(k_match_bf<4>, grid(BM_QUERIES(4)), block, 0, st, args...);
}

static orbfe_status launch_bf(int kernel, int tiles, const uint8_t *d_q, int nq, const uint8_t *d_t, int nt, const float *d_qa,
                              const float *d_ta, int ang_stride, float nnratio, int th, int check_ori,
                              int32_t *d_match, int32_t *d_best, int32_t *d_second, int32_t *d_nm, hipStream_t st)
{
    if (nq > 0) {
        if (kernel == 1)
            hipLaunchKernelGGL(k_match_popc, dim3((nq + 255) / 256, 1), dim3(256), 0, st, d_q, d_t, (const int32_t *)nullptr,
                               (const int32_t *)nullptr, (const int32_t *)nullptr, (const int32_t *)nullptr, 0, nq, nt, nnratio, th,
                               d_match, d_best, d_second);
        else
            launch_match_bf(tiles, nq, 1, st, d_q, d_t, (const int32_t *)nullptr, (const int32_t *)nullptr, (const int32_t *)nullptr,
                            (const int32_t *)nullptr, 0, nq, nt, nnratio, th, d_match, d_best, d_second);
        ORBFE_HIP(hipGetLastError());
    }
    const int ori = (check_ori && d_qa && d_ta) ? 1 : 0;
    hipLaunchKernelGGL(k_rot_prune, dim3(1), dim3(256), 0, st, d_match, d_qa, d_ta, ang_stride,
                       (const int32_t *)nullptr, (const int32_t *)nullptr, (const int32_t *)nullptr, 0, nq, ori, d_nm);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_match_bf_device(orbfe_matcher *m, const uint8_t *d_q, int32_t nq, const uint8_t *d_t,
                                              int32_t nt, const float *d_q_angle, const float *d_t_angle,
                                              float nnratio, int32_t th, int32_t check_ori, int32_t *d_match_q2t,
                                              int32_t *d_best, int32_t *d_second, int32_t *d_nmatches, void *stream)
{
    if (!m || nq < 0 || nt < 0 || nt > BM_MAX_NT || !d_match_q2t || !d_nmatches || (nq > 0 && !d_q) || (nt > 0 && !d_t)) {
        orbfe_set_error("bad argument to orbfe_match_bf_device (train set limited to %d descriptors)", BM_MAX_NT);
        return ORBFE_ERR_ARG;
    }
    DeviceGuard g(m->device);
    return launch_bf(m->bf_kernel, m->bf_tiles, d_q, nq, d_t, nt, d_q_angle, d_t_angle, 1, nnratio, th, check_ori, d_match_q2t, d_best, d_second,
                     d_nmatches, (hipStream_t)stream);
}

extern "C" orbfe_status orbfe_match_bf(orbfe_matcher *m, const uint8_t *q, int32_t nq, const uint8_t *t, int32_t nt,
                                       const float *q_angle, const float *t_angle, float nnratio, int32_t th,
                                       int32_t check_ori, int32_t *match_q2t, int32_t *best, int32_t *second,
                                       int32_t *nmatches)
{
    if (!m || nq < 0 || nt < 0 || nt > BM_MAX_NT || (nq > 0 && (!q || !match_q2t)) || (nt > 0 && !t)) {
        orbfe_set_error("bad argument to orbfe_match_bf (train set limited to %d descriptors)", BM_MAX_NT);
        return ORBFE_ERR_ARG;
    }
    if (nq == 0) {
        if (nmatches) *nmatches = 0;
        return ORBFE_OK;
    }
    DeviceGuard g(m->device);
    hipStream_t st = m->stream;
    ORBFE_HIP(scratch_acquire(m, st));  // a device-buffer call on another stream may still be using the scratch blocks
    const bool ori = check_ori && q_angle && t_angle;
    ORBFE_HIP(m->b[0].ensure((size_t)nq * 32));
    ORBFE_HIP(m->b[1].ensure((size_t)nt * 32));
    ORBFE_HIP(m->b[2].ensure((size_t)nq * 4));
    ORBFE_HIP(m->b[3].ensure((size_t)nt * 4));
    ORBFE_HIP(m->b[4].ensure((size_t)nq * 4));
    ORBFE_HIP(m->b[5].ensure((size_t)nq * 4));
    ORBFE_HIP(m->b[6].ensure((size_t)nq * 4));
    ORBFE_HIP(m->b[7].ensure(4));
    ORBFE_HIP(hipMemcpyAsync(m->b[0].p, q, (size_t)nq * 32, hipMemcpyHostToDevice, st));
    if (nt > 0) ORBFE_HIP(hipMemcpyAsync(m->b[1].p, t, (size_t)nt * 32, hipMemcpyHostToDevice, st));
    if (ori) {
        ORBFE_HIP(hipMemcpyAsync(m->b[2].p, q_angle, (size_t)nq * 4, hipMemcpyHostToDevice, st));
        if (nt > 0) ORBFE_HIP(hipMemcpyAsync(m->b[3].p, t_angle, (size_t)nt * 4, hipMemcpyHostToDevice, st));
    }
    orbfe_status s = launch_bf(m->bf_kernel, m->bf_tiles, m->b[0].as<const uint8_t>(), nq, m->b[1].as<const uint8_t>(), nt,
                               ori ? m->b[2].as<const float>() : nullptr, ori ? m->b[3].as<const float>() : nullptr, 1,
                               nnratio, th, ori ? 1 : 0, m->b[4].as<int32_t>(), m->b[5].as<int32_t>(),
                               m->b[6].as<int32_t>(), m->b[7].as<int32_t>(), st);
    if (s != ORBFE_OK) return s;
    int32_t nm = 0;
    ORBFE_HIP(hipMemcpyAsync(match_q2t, m->b[4].p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    if (best) ORBFE_HIP(hipMemcpyAsync(best, m->b[5].p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    if (second) ORBFE_HIP(hipMemcpyAsync(second, m->b[6].p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipMemcpyAsync(&nm, m->b[7].p, 4, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    if (nmatches) *nmatches = nm;
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_match_bf_blocks_device(orbfe_matcher *m, const orbfe_keypoint *d_qkps, const uint8_t *d_qdesc,
                                                     const int32_t *d_qn, const orbfe_keypoint *d_tkps, const uint8_t *d_tdesc,
                                                     const int32_t *d_tn, int32_t cap, const int32_t *d_qframe,
                                                     const int32_t *d_tframe, int32_t npairs, float nnratio, int32_t th,
                                                     int32_t check_ori, int32_t *d_match_q2t, int32_t *d_nmatches, void *stream)
{
    return orbfe_internal_match_bf_blocks_tiles(m, d_qkps, d_qdesc, d_qn, d_tkps, d_tdesc, d_tn, cap, d_qframe, d_tframe, npairs, nnratio, th,
                                                check_ori, d_match_q2t, d_nmatches, m ? m->bf_tiles : 0, stream);
}

// orbfe_match_bf_blocks_device with the query tiles per wave of k_match_bf given by the call (the pipeline's lane calls) instead of
// by the handle
orbfe_status orbfe_internal_match_bf_blocks_tiles(orbfe_matcher *m, const orbfe_keypoint *d_qkps, const uint8_t *d_qdesc,
                                                  const int32_t *d_qn, const orbfe_keypoint *d_tkps, const uint8_t *d_tdesc,
                                                  const int32_t *d_tn, int32_t cap, const int32_t *d_qframe, const int32_t *d_tframe,
                                                  int32_t npairs, float nnratio, int32_t th, int32_t check_ori, int32_t *d_match_q2t,
                                                  int32_t *d_nmatches, int32_t tiles, void *stream)
{
    if (!m || !d_qkps || !d_qdesc || !d_qn || !d_tkps || !d_tdesc || !d_tn || !d_qframe || !d_tframe || !d_match_q2t ||
        !d_nmatches || cap < 1 || cap > BM_MAX_NT || npairs < 0 || !orb_match_tiles_ok(tiles)) {
        orbfe_set_error("bad argument to orbfe_match_bf_blocks_device / _frames_device (cap 1..%d)", BM_MAX_NT);
        return ORBFE_ERR_ARG;
    }
    if (npairs == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    hipStream_t st = (hipStream_t)stream;
    if (m->bf_kernel == 1)
        hipLaunchKernelGGL(k_match_popc, dim3((cap + 255) / 256, npairs), dim3(256), 0, st, d_qdesc, d_tdesc, d_qn, d_tn, d_qframe,
                           d_tframe, cap, 0, 0, nnratio, th, d_match_q2t, (int32_t *)nullptr, (int32_t *)nullptr);
    else
        launch_match_bf(tiles, cap, npairs, st, d_qdesc, d_tdesc, d_qn, d_tn, d_qframe, d_tframe, cap, 0, 0, nnratio, th, d_match_q2t,
                        (int32_t *)nullptr, (int32_t *)nullptr);
    ORBFE_HIP(hipGetLastError());
    // orbfe_keypoint.angle, stride 7 floats
    hipLaunchKernelGGL(k_rot_prune, dim3(npairs), dim3(256), 0, st, d_match_q2t, &d_qkps->angle, &d_tkps->angle, 7, d_qn, d_qframe,
                       d_tframe, cap, 0, check_ori ? 1 : 0, d_nmatches);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_match_bf_frames_device(orbfe_matcher *m, const orbfe_keypoint *d_kps,
                                                     const uint8_t *d_desc, const int32_t *d_n, int32_t cap,
                                                     const int32_t *d_qframe, const int32_t *d_tframe, int32_t npairs,
                                                     float nnratio, int32_t th, int32_t check_ori,
                                                     int32_t *d_match_q2t, int32_t *d_nmatches, void *stream)
{
    return orbfe_match_bf_blocks_device(m, d_kps, d_desc, d_n, d_kps, d_desc, d_n, cap, d_qframe, d_tframe, npairs, nnratio, th,
                                        check_ori, d_match_q2t, d_nmatches, stream);
}

extern "C" orbfe_status orbfe_hamming_csr_ex(orbfe_matcher *m, const uint8_t *q, int32_t nq, const uint8_t *t, int32_t nt,
                                             const uint32_t *off, const uint32_t *cand, int32_t *best_idx, int32_t *best,
                                             int32_t *second, int32_t *second_idx)
{
    if (!m || nq < 0 || nt < 0 || (nq > 0 && (!q || !off || !best_idx || !best || !second))) {
        orbfe_set_error("bad argument to orbfe_hamming_csr");
        return ORBFE_ERR_ARG;
    }
    if (nq == 0) return ORBFE_OK;
    const size_t nc = off[nq];
    for (int i = 0; i < nq; ++i)
        if (off[i + 1] < off[i]) { orbfe_set_error("CSR offsets must not decrease"); return ORBFE_ERR_ARG; }
    for (size_t k = 0; k < nc; ++k)
        if (cand[k] >= (uint32_t)nt) { orbfe_set_error("candidate index out of range"); return ORBFE_ERR_ARG; }
    DeviceGuard g(m->device);
    hipStream_t st = m->stream;
    ORBFE_HIP(scratch_acquire(m, st));  // a device-buffer call on another stream may still be using the scratch blocks
    ORBFE_HIP(m->b[0].ensure((size_t)nq * 32));
    ORBFE_HIP(m->b[1].ensure((size_t)nt * 32));
    ORBFE_HIP(m->b[2].ensure((size_t)(nq + 1) * 4));
    ORBFE_HIP(m->b[3].ensure(nc * 4));
    ORBFE_HIP(m->b[4].ensure((size_t)nq * 4));
    ORBFE_HIP(m->b[5].ensure((size_t)nq * 4));
    ORBFE_HIP(m->b[6].ensure((size_t)nq * 4));
    ORBFE_HIP(m->b[7].ensure((size_t)nq * 4));
    ORBFE_HIP(hipMemcpyAsync(m->b[0].p, q, (size_t)nq * 32, hipMemcpyHostToDevice, st));
    if (nt > 0) ORBFE_HIP(hipMemcpyAsync(m->b[1].p, t, (size_t)nt * 32, hipMemcpyHostToDevice, st));
    ORBFE_HIP(hipMemcpyAsync(m->b[2].p, off, (size_t)(nq + 1) * 4, hipMemcpyHostToDevice, st));
    if (nc > 0) ORBFE_HIP(hipMemcpyAsync(m->b[3].p, cand, nc * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_hamming_csr, dim3((nq + 255) / 256), dim3(256), 0, st, m->b[0].as<const uint8_t>(), nq,
                       m->b[1].as<const uint8_t>(), m->b[2].as<const uint32_t>(), m->b[3].as<const uint32_t>(),
                       m->b[4].as<int32_t>(), m->b[5].as<int32_t>(), m->b[6].as<int32_t>(), m->b[7].as<int32_t>());
    ORBFE_HIP(hipGetLastError());
    if (second_idx) ORBFE_HIP(hipMemcpyAsync(second_idx, m->b[7].p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipMemcpyAsync(best_idx, m->b[4].p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipMemcpyAsync(best, m->b[5].p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipMemcpyAsync(second, m->b[6].p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_hamming_csr_all(orbfe_matcher *m, const uint8_t *q, int32_t nq, const uint8_t *t, int32_t nt,
                                              const uint32_t *off, const uint32_t *cand, uint16_t *dist)
{
    if (!m || nq < 0 || nt < 0 || (nq > 0 && (!q || !off))) {
        orbfe_set_error("bad argument to orbfe_hamming_csr_all");
        return ORBFE_ERR_ARG;
    }
    if (nq == 0) return ORBFE_OK;
    const size_t nc = off[nq];
    for (int i = 0; i < nq; ++i)
        if (off[i + 1] < off[i]) { orbfe_set_error("CSR offsets must not decrease"); return ORBFE_ERR_ARG; }
    if (nc == 0) return ORBFE_OK;
    if (!cand || !dist || !t) { orbfe_set_error("bad argument to orbfe_hamming_csr_all"); return ORBFE_ERR_ARG; }
    for (size_t k = 0; k < nc; ++k)
        if (cand[k] >= (uint32_t)nt) { orbfe_set_error("candidate index out of range"); return ORBFE_ERR_ARG; }
    DeviceGuard g(m->device);
    hipStream_t st = m->stream;
    ORBFE_HIP(scratch_acquire(m, st));
    ORBFE_HIP(m->b[0].ensure((size_t)nq * 32));
    ORBFE_HIP(m->b[1].ensure((size_t)nt * 32));
    ORBFE_HIP(m->b[2].ensure((size_t)(nq + 1) * 4));
    ORBFE_HIP(m->b[3].ensure(nc * 4));
    ORBFE_HIP(m->b[4].ensure(nc * 2));
    ORBFE_HIP(hipMemcpyAsync(m->b[0].p, q, (size_t)nq * 32, hipMemcpyHostToDevice, st));
    ORBFE_HIP(hipMemcpyAsync(m->b[1].p, t, (size_t)nt * 32, hipMemcpyHostToDevice, st));
    ORBFE_HIP(hipMemcpyAsync(m->b[2].p, off, (size_t)(nq + 1) * 4, hipMemcpyHostToDevice, st));
    ORBFE_HIP(hipMemcpyAsync(m->b[3].p, cand, nc * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_hamming_csr_all, dim3((nq + 3) / 4), dim3(256), 0, st, m->b[0].as<const uint8_t>(), nq,
                       m->b[1].as<const uint8_t>(), m->b[2].as<const uint32_t>(), m->b[3].as<const uint32_t>(), m->b[4].as<uint16_t>());
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipMemcpyAsync(dist, m->b[4].p, nc * 2, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_hamming_csr(orbfe_matcher *m, const uint8_t *q, int32_t nq, const uint8_t *t, int32_t nt,
                                          const uint32_t *off, const uint32_t *cand, int32_t *best_idx, int32_t *best,
                                          int32_t *second)
{
    return orbfe_hamming_csr_ex(m, q, nq, t, nt, off, cand, best_idx, best, second, nullptr);
}

// device-resident form: everything already in HBM (e.g. descriptors of an extractor output block), enqueued on `stream`
extern "C" orbfe_status orbfe_hamming_csr_device(orbfe_matcher *m, const uint8_t *d_q, int32_t nq, const uint8_t *d_t,
                                                 const uint32_t *d_off, const uint32_t *d_cand, int32_t *d_best_idx,
                                                 int32_t *d_best, int32_t *d_second, int32_t *d_second_idx, void *stream)
{
    if (!m || nq < 0 || (nq > 0 && (!d_q || !d_t || !d_off || !d_cand || !d_best_idx || !d_best || !d_second))) {
        orbfe_set_error("bad argument to orbfe_hamming_csr_device");
        return ORBFE_ERR_ARG;
    }
    if (nq == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    hipLaunchKernelGGL(k_hamming_csr, dim3((nq + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_q, nq, d_t, d_off, d_cand,
                       d_best_idx, d_best, d_second, d_second_idx);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}
