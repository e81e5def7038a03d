// orbfe_pnp.hip -- the reference's PnPsolver (src/PnPsolver.cc: EPnP on four correspondences inside a RANSAC loop, Refine's EPnP
// over the best inliers) on the GPU, one solver or a batch.  The arithmetic is csrc/orbfe_epnp.h over csrc/orbfe_svd.h, which
// restate tests/pnp_oracle.py operation for operation: fp64 where the C++ uses double, float where it uses float, no FMA
// (-ffp-contract=off), sums in the C++ order, nothing from libm but IEEE sqrt and division.  So the pose, the masks and every tap
// are bit-exact against the oracle.  Layout: DESIGN.md section 8h.
//   k_pnp_ransac   one workgroup per set.  A chunk is up to PN_K iterations: lane h replays its four draws, gathers its four
//                  correspondences and runs one compute_pose (workspace in the lane's private memory); the workgroup counts
//                  every hypothesis's inliers, points across lanes, one ballot per hypothesis and wave; then the workgroup walks
//                  the chunk in iteration order with the acceptance rule of `iterate`: a new best rewrites the best mask, and
//                  Refine runs once per best mask, cooperatively: per-point steps one point per lane, every sum one entry per
//                  lane walking the inliers in index order, the SVDs and beta solves on lane 0.
//   k_pnp_prepare  the constructor: ordered compaction of the keypoints that have a usable map point.
// The handle, its taps and the host form's round trip are csrc/orbfe_ransac.h; here are the solver's own arrays, the argument
// checks and the kernels.
#include <float.h>
#include <math.h>

#include "orbfe_common.h"
#include "orbfe_ransac.h"
#include "orbfe_epnp.h"

namespace {

constexpr int PN_K = 64;    // hypotheses per chunk: one wave, one lane each
constexpr int PN_T = 256;   // k_pnp_ransac workgroup
constexpr int PN_MAX_ITERATIONS = 1 << 20;
constexpr int PN_SLAB = 13;   // doubles of Refine's workspace per correspondence: pws 3, us 2, alphas 4, pcs 3, reprojection term 1

// the four swap-with-back / pop-back selections out of a fresh 0 .. n-1 (n >= 4) without the list: only the positions that took
// the back element differ from their index, and a later write to a position hides an earlier one
__device__ inline void quad_from_draws(const int32_t *d, int n, int *quad)
{
    int pos[4], val[4];
    for (int k = 0; k < 4; k++) {
        const int size = n - k;
        const int p = index_from_draw(d[k], size);
        int pick = p, back = size - 1;
        for (int e = 0; e < k; e++) {   // in the order written: the last match stays
            if (pos[e] == p) pick = val[e];
            if (pos[e] == size - 1) back = val[e];
        }
        quad[k] = pick;
        pos[k] = p;
        val[k] = back;
    }
}

struct PnHyp {
    double R[9], t[3];
};

struct PnPoint {
    double X[3];
    float u, v, thr;
};

__device__ inline void load_point(const float *P3, const float *P2, const float *sig, float th2, int i, PnPoint &p)
{
    for (int k = 0; k < 3; k++) p.X[k] = (double)P3[3 * (size_t)i + k];
    p.u = P2[2 * (size_t)i];
    p.v = P2[2 * (size_t)i + 1];
    p.thr = sig[i] * th2;
}

// CheckInliers for one point (oracle P8)
__device__ inline bool check_point(const PnPoint &p, const PnHyp &h, const double *K, float &error2)
{
    const float Xc = (float)(h.R[0] * p.X[0] + h.R[1] * p.X[1] + h.R[2] * p.X[2] + h.t[0]);
    const float Yc = (float)(h.R[3] * p.X[0] + h.R[4] * p.X[1] + h.R[5] * p.X[2] + h.t[1]);
    const float invZc = (float)(1 / (h.R[6] * p.X[0] + h.R[7] * p.X[1] + h.R[8] * p.X[2] + h.t[2]));
    const double ue = K[2] + K[0] * Xc * invZc;
    const double ve = K[3] + K[1] * Yc * invZc;
    const float distX = (float)(p.u - ue);
    const float distY = (float)(p.v - ve);
    error2 = distX * distX + distY * distY;
    return error2 < p.thr;
}

struct PnArgs {
    const int32_t *off;
    const float *P3, *P2, *sig;
    const orbfe_pnp_set *sets;
    const int32_t *draws;
    orbfe_pnp_state *state;
    uint8_t *best_mask;
    orbfe_pnp_result *result;
    uint8_t *mask;
    const int32_t *kp_index;
    uint8_t *key_mask;
    double *slab;      // [max_points][PN_SLAB]: Refine's per-correspondence workspace
    int32_t *ridx;     // [max_points]: Refine's index list
    int max_points;    // bounds all sets of a batch together
    orbfe_pnp_iter *tap_iter;   // [tap_sets][ORBFE_PNP_TAP_ITERS]
    float *tap_err;             // [tap_sets][max_points]
    int32_t *tap_info;          // [tap_sets][2]: iterations run, points of the set
    int tap_sets, tap_iteration;
};

__device__ inline void tcw_from(float *T, const PnHyp &h)
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T[4 * i + j] = (float)h.R[3 * i + j];
        T[4 * i + 3] = (float)h.t[i];
    }
    T[12] = T[13] = T[14] = 0.0f;
    T[15] = 1.0f;
}

// ---- RANSAC --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PN_T) void k_pnp_ransac(PnArgs a)
{
    __shared__ PnHyp sH[PN_K], sBest, sRef;
    __shared__ int sQuad[PN_K][4], sN[PN_K], sCnt[PN_K];
    __shared__ double sMtM[144], sCws[12], sS3[9], sCi[9], sCcs[4][3], sPc0[3], sPw0[3], sAbt[9], sRep[4];
    __shared__ PnHyp sRt[4];
    __shared__ int sRefCnt, sRefN;
    const int set = blockIdx.x, tid = threadIdx.x;
    const int o = a.off[set], n = a.off[set + 1] - o;
    const orbfe_pnp_set P = a.sets[set];
    const bool tapped = set < a.tap_sets;
    orbfe_pnp_result *res = a.result + set;
    if (tapped && tid == 0) {
        a.tap_info[2 * set] = 0;
        a.tap_info[2 * set + 1] = 0;
    }
    auto nothing = [&]() {
        res->found = 0;
        res->no_more = 1;
        res->n_inliers = 0;
        res->iterations_run = 0;
        res->refined = 0;
        res->refine_runs = 0;
        res->reserved[0] = res->reserved[1] = 0;
        for (int e = 0; e < 16; e++) res->Tcw[e] = 0.0f;
    };
    if (n < 0 || o < 0 || (long long)o + n > a.max_points) {   // nothing but the result is written
        if (tid == 0) nothing();
        return;
    }
    orbfe_pnp_state *state = a.state + set;
    uint8_t *mask = a.mask + o, *best_mask = a.best_mask + o;
    uint8_t *key_mask = a.key_mask && a.kp_index && P.n_keys > 0 ? a.key_mask + P.key_offset : nullptr;
    // vbInliers.clear() / vector<bool>(size, false)
    for (int i = tid; i < n; i += PN_T) mask[i] = 0;
    if (key_mask)
        for (int i = tid; i < P.n_keys; i += PN_T) key_mask[i] = 0;
    const int min_inl = P.params.min_inliers, max_its = P.params.max_its;
    if (n < min_inl || n < 4) {
        if (tid == 0) nothing();
        return;
    }
    const float *P3 = a.P3 + 3 * (size_t)o, *P2 = a.P2 + 2 * (size_t)o, *sig = a.sig + o;
    double *slab = a.slab + (size_t)o * PN_SLAB;
    double *r_pws = slab, *r_us = slab + 3 * (size_t)n, *r_al = slab + 5 * (size_t)n, *r_pcs = slab + 9 * (size_t)n, *r_err = slab + 12 * (size_t)n;
    int32_t *ridx = a.ridx + o;
    const double K[4] = {(double)P.K[0], (double)P.K[1], (double)P.K[2], (double)P.K[3]};
    const float th2 = P.params.th2;
    // every lane carries the scan's state: it is a function of what all of them read from LDS
    int iters = state->iterations, best_inl = state->best_inliers;
    const int total = max(P.n_iterations, max_its - iters);   // while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations)
    int run = 0, found = 0, changed = 0, memo = 0, ref_cnt = 0, refine_runs = 0;
    double wsA[144], wsV[144];   // the lane's SVD workspace (private memory)
    double l_6x10[60], rho[6];   // lane 0's, across the steps of Refine
    if (tid == 0) sRefCnt = 0;
    __syncthreads();
    for (int base = 0; base < total && !found; base += PN_K) {
        const int cnt = min(PN_K, total - base);
        if (tid < cnt) {
            int quad[4];
            quad_from_draws(a.draws + P.draws_offset + 4 * (size_t)(base + tid), n, quad);
            double pws[12], us[8], al[16], pcs[12], rep[3];
            for (int j = 0; j < 4; j++) {
                for (int k = 0; k < 3; k++) pws[3 * j + k] = (double)P3[3 * (size_t)quad[j] + k];
                us[2 * j] = (double)P2[2 * (size_t)quad[j]];
                us[2 * j + 1] = (double)P2[2 * (size_t)quad[j] + 1];
            }
            PnHyp h;
            int N;
            epnp_compute_pose(4, pws, us, al, pcs, K, wsA, wsV, h.R, h.t, &N, rep);
            sH[tid] = h;
            for (int j = 0; j < 4; j++) sQuad[tid][j] = quad[j];
            sN[tid] = N;
            sCnt[tid] = 0;
        }
        __syncthreads();
        // inlier counts: integer sums, any order
        for (int i0 = 0; i0 < n; i0 += PN_T) {
            const int i = i0 + tid;
            const bool valid = i < n;
            PnPoint p;
            if (valid) load_point(P3, P2, sig, th2, i, p);
            for (int h = 0; h < cnt; h++) {
                float e2 = 0;
                const bool in = valid && check_point(p, sH[h], K, e2);
                const unsigned long long b = __ballot(in);
                if ((tid & 63) == 0 && b) atomicAdd(&sCnt[h], __popcll(b));
                if (tapped && valid && base + h == a.tap_iteration) a.tap_err[(size_t)set * a.max_points + i] = e2;
            }
        }
        __syncthreads();
        // the serial loop over the chunk, the whole workgroup in step
        for (int h = 0; h < cnt; h++) {
            iters++;
            run++;
            const int c = sCnt[h];
            int ran = 0;
            if (c >= min_inl) {
                if (c > best_inl) {   // strict: a tie keeps the earlier best
                    best_inl = c;
                    changed = 1;
                    memo = 0;
                    if (tid == 0) sBest = sH[h];
                    for (int i = tid; i < n; i += PN_T) {
                        PnPoint p;
                        load_point(P3, P2, sig, th2, i, p);
                        float e2;
                        best_mask[i] = check_point(p, sH[h], K, e2);
                    }
                    __syncthreads();
                }
                if (!memo) {   // Refine(): a function of mvbBestInliers alone
                    ran = 1;
                    refine_runs++;
                    if (tid == 0) {
                        int m = 0;
                        for (int i = 0; i < n; i++)
                            if (best_mask[i]) ridx[m++] = i;
                        sRefN = m;
                        sRefCnt = 0;
                    }
                    __syncthreads();
                    const int m = sRefN;
                    for (int q = tid; q < m; q += PN_T) {
                        const int i = ridx[q];
                        for (int k = 0; k < 3; k++) r_pws[3 * (size_t)q + k] = (double)P3[3 * (size_t)i + k];
                        r_us[2 * (size_t)q] = (double)P2[2 * (size_t)i];
                        r_us[2 * (size_t)q + 1] = (double)P2[2 * (size_t)i + 1];
                    }
                    __syncthreads();
                    // compute_pose over the best inliers, the pieces of csrc/orbfe_epnp.h spread over the workgroup: one point per
                    // lane, or one entry of a sum per lane walking the inliers in index order (no tree reductions)
                    if (tid < 3) sCws[tid] = epnp_col_sum(m, r_pws, 3, tid) / m;
                    __syncthreads();
                    if (tid < 6) {
                        const int i = tid < 3 ? 0 : tid < 5 ? 1 : 2, j = tid < 3 ? tid : tid < 5 ? tid - 2 : 2;
                        sS3[3 * i + j] = sS3[3 * j + i] = epnp_pw0_entry(m, r_pws, sCws, i, j);
                    }
                    __syncthreads();
                    if (tid == 0) {
                        double cws[4][3], ci[9];
                        for (int e = 0; e < 3; e++) cws[0][e] = sCws[e];
                        epnp_control_points(m, sS3, cws, ci);
                        for (int e = 0; e < 12; e++) sCws[e] = cws[e / 3][e % 3];
                        for (int e = 0; e < 9; e++) sCi[e] = ci[e];
                    }
                    __syncthreads();
                    for (int q = tid; q < m; q += PN_T) epnp_alpha_point(r_pws + 3 * (size_t)q, sCws, sCi, r_al + 4 * (size_t)q);
                    __syncthreads();
                    if (tid < 78) {   // the upper triangle of M^T M
                        int i = 0, e = tid;
                        while (e >= 12 - i) e -= 12 - i, i++;
                        const int j = i + e;
                        sMtM[12 * i + j] = sMtM[12 * j + i] = epnp_mtm_entry(m, r_al, r_us, K, i, j);
                    }
                    __syncthreads();
                    if (tid == 0) {
                        double cws[4][3];
                        for (int e = 0; e < 12; e++) cws[e / 3][e % 3] = sCws[e];
                        for (int e = 0; e < 144; e++) wsA[e] = sMtM[e];
                        epnp_nullspace(wsA, wsV, cws, l_6x10, rho);
                    }
                    for (int k = 1; k <= 3; k++) {
                        if (tid == 0) {
                            double ccs[4][3];
                            epnp_betas_ccs(k, l_6x10, rho, wsA, ccs);
                            for (int e = 0; e < 12; e++) sCcs[e / 3][e % 3] = ccs[e / 3][e % 3];
                        }
                        __syncthreads();
                        for (int q = tid; q < m; q += PN_T) epnp_pc_point(r_al + 4 * (size_t)q, sCcs, r_pcs + 3 * (size_t)q);
                        __syncthreads();
                        const bool flip = r_pcs[2] < 0.0;   // solve_for_sign reads the first point only
                        __syncthreads();
                        if (flip)
                            for (int q = tid; q < 3 * m; q += PN_T) r_pcs[q] = -r_pcs[q];
                        __syncthreads();
                        if (tid < 3)
                            sPc0[tid] = epnp_col_sum(m, r_pcs, 3, tid) / m;
                        else if (tid < 6)
                            sPw0[tid - 3] = epnp_col_sum(m, r_pws, 3, tid - 3) / m;
                        __syncthreads();
                        if (tid < 9) sAbt[tid] = epnp_abt_entry(m, r_pcs, r_pws, sPc0, sPw0, tid / 3, tid % 3);
                        __syncthreads();
                        if (tid == 0) epnp_R_t_from_abt(sAbt, sPc0, sPw0, sRt[k].R, sRt[k].t);
                        __syncthreads();
                        for (int q = tid; q < m; q += PN_T)
                            r_err[q] = epnp_reproj_term(r_pws + 3 * (size_t)q, r_us[2 * (size_t)q], r_us[2 * (size_t)q + 1], K, sRt[k].R, sRt[k].t);
                        __syncthreads();
                        if (tid == 0) {   // the sum is serial, in index order
                            double sum2 = 0.0;
                            for (int q = 0; q < m; q++) sum2 += r_err[q];
                            sRep[k] = sum2 / m;
                        }
                    }
                    if (tid == 0) sRef = sRt[epnp_choose(sRep)];
                    __syncthreads();
                    for (int i0 = 0; i0 < n; i0 += PN_T) {
                        const int i = i0 + tid;
                        bool in = false;
                        if (i < n) {
                            PnPoint p;
                            load_point(P3, P2, sig, th2, i, p);
                            float e2;
                            in = check_point(p, sRef, K, e2);
                            mask[i] = in;   // vbInliers if this Refine returns; cleared below if not
                        }
                        const unsigned long long b = __ballot(in);
                        if ((tid & 63) == 0 && b) atomicAdd(&sRefCnt, __popcll(b));
                    }
                    __syncthreads();
                    ref_cnt = sRefCnt;
                    memo = 1;
                }
                if (ref_cnt > min_inl) found = 1;
            }
            if (tapped && tid == 0 && base + h < ORBFE_PNP_TAP_ITERS) {
                orbfe_pnp_iter *ti = a.tap_iter + (size_t)set * ORBFE_PNP_TAP_ITERS + base + h;
                for (int j = 0; j < 4; j++) ti->quad[j] = sQuad[h][j];
                ti->N = sN[h];
                ti->n_inliers = c;
                ti->refine_ran = ran;
                ti->refine_inliers = c >= min_inl ? ref_cnt : 0;
                for (int e = 0; e < 9; e++) ti->R[e] = sH[h].R[e];
                for (int e = 0; e < 3; e++) ti->t[e] = sH[h].t[e];
            }
            if (found) break;   // hypotheses past a return are discarded
        }
        __syncthreads();
    }
    // a return of Refine leaves its mask in place; at the clamp the best model goes out with the best mask; else no model
    const bool at_clamp = !found && iters >= max_its;
    const bool best_out = at_clamp && best_inl >= min_inl;
    if (!found)
        for (int i = tid; i < n; i += PN_T) mask[i] = best_out ? best_mask[i] : 0;
    __syncthreads();
    if ((found || best_out) && key_mask)
        for (int i = tid; i < n; i += PN_T)
            if (mask[i]) {
                const int k = a.kp_index[o + i];
                if (k >= 0 && k < P.n_keys) key_mask[k] = 1;
            }
    if (tid == 0) {
        state->iterations = iters;
        state->best_inliers = best_inl;
        if (changed) tcw_from(state->best_Tcw, sBest);
        res->found = found || best_out;
        res->no_more = at_clamp;
        res->n_inliers = found ? ref_cnt : best_out ? best_inl : 0;
        res->iterations_run = run;
        res->refined = found;
        res->refine_runs = refine_runs;
        res->reserved[0] = res->reserved[1] = 0;
        if (found)
            tcw_from(res->Tcw, sRef);
        else
            for (int e = 0; e < 16; e++) res->Tcw[e] = best_out ? state->best_Tcw[e] : 0.0f;
        if (tapped) {
            a.tap_info[2 * set] = run;
            a.tap_info[2 * set + 1] = n;
        }
    }
}

// ---- the constructor on device data ------------------------------------------------------------------------------------------------
// One workgroup walks the keypoints in chunks of PN_T and keeps those with a usable map point, in keypoint order: ballot prefix
// inside a wave, the waves' totals through LDS, a running base across chunks.
struct PnKeyPoint {   // cv::KeyPoint as the extractor writes it (KP record, 28 bytes)
    float x, y, size, angle, response;
    int32_t octave, class_id;
};

__global__ __launch_bounds__(PN_T) void k_pnp_prepare(const PnKeyPoint *keys, int n_keys, const float *level_sigma2, int n_levels,
                                                       const int32_t *mp_index, const float *mp_pos, int n_mp, float *P2D, float *sigma2,
                                                       float *P3Dw, int32_t *kp_index, int32_t *count, int cap)
{
    __shared__ int sWave[PN_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int i0 = 0; i0 < n_keys; i0 += PN_T) {
        const int i = i0 + tid;
        int m = -1, oct = 0;
        if (i < n_keys) {
            m = mp_index[i];
            oct = keys[i].octave;
            if (m >= n_mp || oct < 0 || oct >= n_levels) m = -1;
        }
        const bool keep = m >= 0;
        const unsigned long long b = __ballot(keep);
        const int before = __popcll(b & ((1ull << lane) - 1));
        if (lane == 0) sWave[wave] = __popcll(b);
        __syncthreads();
        int wbase = 0, total = 0;
        for (int w = 0; w < PN_T / 64; w++) {
            if (w < wave) wbase += sWave[w];
            total += sWave[w];
        }
        const int dst = base + wbase + before;
        if (keep && dst < cap) {
            P2D[2 * (size_t)dst] = keys[i].x;
            P2D[2 * (size_t)dst + 1] = keys[i].y;
            sigma2[dst] = level_sigma2[oct];
            for (int k = 0; k < 3; k++) P3Dw[3 * (size_t)dst + k] = mp_pos[3 * (size_t)m + k];
            kp_index[dst] = i;
        }
        base += total;
        __syncthreads();
    }
    if (tid == 0) *count = base < cap ? base : cap;
}

// ---- known-answer kernels ------------------------------------------------------------------------------------------------------
__global__ void k_pnp_kat(int what, int n, const double *in, double *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int id, od;
    epnp_kat_sizes(what, &id, &od);
    double ws[300];
    epnp_kat_item(what, in + (size_t)i * id, out + (size_t)i * od, ws);
}

// one compute_pose; ws: n * PN_SLAB doubles
__global__ void k_pnp_kat_pose(int n, const double *in, double *out, double *ws)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double *pws = ws, *us = ws + 3 * (size_t)n, *al = ws + 5 * (size_t)n, *pcs = ws + 9 * (size_t)n;
    for (int i = 0; i < n; i++) {
        for (int j = 0; j < 3; j++) pws[3 * (size_t)i + j] = in[4 + 5 * (size_t)i + j];
        us[2 * (size_t)i] = in[4 + 5 * (size_t)i + 3];
        us[2 * (size_t)i + 1] = in[4 + 5 * (size_t)i + 4];
    }
    double A[144], V[144];
    int N;
    out[12] = epnp_compute_pose(n, pws, us, al, pcs, in, A, V, out, out + 9, &N, out + 14);
    out[13] = (double)N;
}

}  // namespace

struct orbfe_pnp : RansacHandle {
    float *d_P3 = nullptr, *d_P2 = nullptr, *d_sig = nullptr;
    double *d_slab = nullptr;
    int32_t *d_ridx = nullptr;
    std::vector<OrbAlloc> blocks(size_t np)
    {
        return {orb_blk(&d_P3, np * 12), orb_blk(&d_P2, np * 8), orb_blk(&d_sig, np * 4), orb_blk(&d_slab, np * PN_SLAB * sizeof(double)),
                orb_blk(&d_ridx, np * 4)};
    }
};

static const RansacSizes PN_SIZES = {sizeof(orbfe_pnp_set), sizeof(orbfe_pnp_state), sizeof(orbfe_pnp_result), sizeof(orbfe_pnp_iter), 1,
                                     ORBFE_PNP_TAP_SETS, ORBFE_PNP_TAP_ITERS};

extern "C" orbfe_status orbfe_pnp_create(int32_t device, int32_t max_points, int32_t max_sets, orbfe_pnp **out)
{
    return ransac_create("orbfe_pnp_create", PN_SIZES, device, max_points, max_sets, out);
}

extern "C" void orbfe_pnp_destroy(orbfe_pnp *h) { orb_destroy(h, ransac_free<orbfe_pnp>); }

extern "C" void *orbfe_pnp_get_stream(orbfe_pnp *h) { return h ? (void *)h->stream : nullptr; }

extern "C" orbfe_status orbfe_pnp_ransac_params(double probability, int32_t min_inliers, int32_t max_its, int32_t min_set, float epsilon,
                                                int32_t n, orbfe_pnp_params *out)
{
    if (!out) return ORBFE_ERR_ARG;
    int32_t n_min = x86_double_to_int((double)((float)n * epsilon));
    if (n_min < min_inliers) n_min = min_inliers;
    if (n_min < min_set) n_min = min_set;
    if (epsilon < (float)n_min / (float)n) epsilon = (float)n_min / (float)n;
    int32_t its;
    if (n_min == n)
        its = 1;
    else
        its = x86_double_to_int(ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3))));
    if (its > max_its) its = max_its;
    if (its < 1) its = 1;
    out->min_inliers = n_min;
    out->max_its = its;
    out->epsilon = epsilon;
    out->th2 = 5.991f;
    return ORBFE_OK;
}

static int64_t pnp_total(const orbfe_pnp_state *state, const orbfe_pnp_params *params, int32_t n_iterations)
{
    const int64_t rest = (int64_t)params->max_its - state->iterations;
    return rest > n_iterations ? rest : n_iterations;
}

extern "C" int32_t orbfe_pnp_iterations(const orbfe_pnp_state *state, const orbfe_pnp_params *params, int32_t n_iterations)
{
    if (!state || !params) return 0;
    const int64_t t = pnp_total(state, params, n_iterations);
    return t < 0 ? 0 : t > INT32_MAX ? INT32_MAX : (int32_t)t;
}

static orbfe_status pnp_launch(orbfe_pnp *h, PnArgs &a, int nsets, hipStream_t st)
{
    a.slab = h->d_slab;
    a.ridx = h->d_ridx;
    ransac_bind_taps(h, a, nsets, st);
    if (nsets == 0) return ORBFE_OK;
    k_pnp_ransac<<<nsets, PN_T, 0, st>>>(a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_pnp_iterate(orbfe_pnp *h, const float *P3Dw, const float *P2D, const float *sigma2, int32_t n, const float *K,
                                          const orbfe_pnp_params *params, int32_t n_iterations, const int32_t *draws,
                                          orbfe_pnp_state *state, uint8_t *best_mask, orbfe_pnp_result *result, uint8_t *mask)
{
    if (!h || !K || !params || !state || !result || n < 0 || (n > 0 && (!P3Dw || !P2D || !sigma2 || !best_mask))) {
        orbfe_set_error("orbfe_pnp_iterate: a required pointer is NULL or n < 0");
        return ORBFE_ERR_ARG;
    }
    if (n > h->max_points) {
        orbfe_set_error("%d correspondences exceed max_points %d", n, h->max_points);
        return ORBFE_ERR_ARG;
    }
    if (params->min_inliers < 0 || state->iterations < 0 || state->best_inliers < 0 || n_iterations < 0) {
        orbfe_set_error("negative n_iterations, min_inliers or state counters");
        return ORBFE_ERR_ARG;
    }
    const bool runs = n >= params->min_inliers && n >= 4;   // else the kernel reads no draw
    const int64_t total = runs ? pnp_total(state, params, n_iterations) : 0;
    if (total > PN_MAX_ITERATIONS || (total > 0 && !draws)) {
        orbfe_set_error("%lld iterations outside [0, %d], or no draws", (long long)total, PN_MAX_ITERATIONS);
        return ORBFE_ERR_ARG;
    }
    DeviceGuard dg(h->device);
    orbfe_pnp_set set = {};
    for (int k = 0; k < 4; k++) set.K[k] = K[k];
    set.params = *params;
    set.n_iterations = n_iterations;
    PnArgs a = {};
    a.P3 = h->d_P3;
    a.P2 = h->d_P2;
    a.sig = h->d_sig;
    return ransac_host_call(h, PN_SIZES, a, pnp_launch, n, &set, state, draws, 4 * (size_t)total,
                            {{h->d_P3, P3Dw, 12}, {h->d_P2, P2D, 8}, {h->d_sig, sigma2, 4}}, best_mask, result, mask);
}

extern "C" orbfe_status orbfe_pnp_iterate_device(orbfe_pnp *h, const int32_t *d_offsets, const float *d_P3Dw, const float *d_P2D,
                                                 const float *d_sigma2, const orbfe_pnp_set *d_sets, const int32_t *d_draws,
                                                 int32_t nsets, orbfe_pnp_state *d_state, uint8_t *d_best_mask,
                                                 orbfe_pnp_result *d_result, uint8_t *d_mask, const int32_t *d_keypoint_index,
                                                 uint8_t *d_key_mask, void *stream)
{
    if (!h || nsets < 0 ||
        (nsets > 0 && (!d_offsets || !d_P3Dw || !d_P2D || !d_sigma2 || !d_sets || !d_draws || !d_state || !d_best_mask || !d_result ||
                       !d_mask))) {
        orbfe_set_error("orbfe_pnp_iterate_device: a required pointer is NULL or nsets < 0");
        return ORBFE_ERR_ARG;
    }
    if ((d_keypoint_index == nullptr) != (d_key_mask == nullptr)) {
        orbfe_set_error("d_keypoint_index and d_key_mask go together");
        return ORBFE_ERR_ARG;
    }
    if (nsets > h->max_sets) {
        orbfe_set_error("%d sets exceed max_sets %d", nsets, h->max_sets);
        return ORBFE_ERR_ARG;
    }
    DeviceGuard dg(h->device);
    PnArgs a = {};
    a.off = d_offsets;
    a.P3 = d_P3Dw;
    a.P2 = d_P2D;
    a.sig = d_sigma2;
    a.sets = d_sets;
    a.draws = d_draws;
    a.state = d_state;
    a.best_mask = d_best_mask;
    a.result = d_result;
    a.mask = d_mask;
    a.kp_index = d_keypoint_index;
    a.key_mask = d_key_mask;
    return pnp_launch(h, a, nsets, (hipStream_t)stream);
}

extern "C" orbfe_status orbfe_pnp_prepare_device(orbfe_pnp *h, const void *d_keys, int32_t n_keys, const float *d_level_sigma2,
                                                 int32_t n_levels, const int32_t *d_mappoint_index, const float *d_mappoint_pos,
                                                 int32_t n_mappoints, float *d_P2D, float *d_sigma2, float *d_P3Dw,
                                                 int32_t *d_keypoint_index, int32_t *d_count, int32_t capacity, void *stream)
{
    if (!h || n_keys < 0 || n_levels < 1 || n_mappoints < 0 || capacity < 0 || !d_count || !d_level_sigma2 ||
        (n_keys > 0 && (!d_keys || !d_mappoint_index || !d_P2D || !d_sigma2 || !d_P3Dw || !d_keypoint_index)) ||
        (n_mappoints > 0 && !d_mappoint_pos)) {
        orbfe_set_error("orbfe_pnp_prepare_device: a required pointer is NULL or a count is negative");
        return ORBFE_ERR_ARG;
    }
    DeviceGuard dg(h->device);
    k_pnp_prepare<<<1, PN_T, 0, (hipStream_t)stream>>>((const PnKeyPoint *)d_keys, n_keys, d_level_sigma2, n_levels, d_mappoint_index,
                                                      d_mappoint_pos, n_mappoints, d_P2D, d_sigma2, d_P3Dw, d_keypoint_index, d_count,
                                                      capacity);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_pnp_set_tap_iteration(orbfe_pnp *h, int32_t iteration)
{
    return ransac_set_tap_iteration(h, PN_SIZES, "orbfe_pnp_set_tap_iteration", iteration);
}

extern "C" orbfe_status orbfe_pnp_tap(orbfe_pnp *h, int32_t set, int32_t stage, void *dst, size_t cap, int32_t *count)
{
    if (!h || !dst || !count || stage < ORBFE_PNP_TAP_ITERATIONS || stage > ORBFE_PNP_TAP_ERRORS) return ORBFE_ERR_ARG;
    return ransac_tap(h, PN_SIZES, set, stage == ORBFE_PNP_TAP_ITERATIONS, dst, cap, count);
}

extern "C" orbfe_status orbfe_pnp_kat(int32_t what, int32_t n, const double *in, double *out)
{
    if (n < 0 || !out || (!in && n > 0) || what < ORBFE_PNP_KAT_SVD3 || what > ORBFE_PNP_KAT_COMPUTE_POSE) return ORBFE_ERR_ARG;
    if (n == 0) return ORBFE_OK;
    const bool pose = what == ORBFE_PNP_KAT_COMPUTE_POSE;
    int id = 0, od = 0;
    if (!pose) epnp_kat_sizes(what, &id, &od);
    const size_t in_b = (pose ? 4 + 5 * (size_t)n : (size_t)n * id) * sizeof(double);
    const size_t out_b = (pose ? 17 : (size_t)n * od) * sizeof(double);
    const size_t ws_b = pose ? (size_t)n * PN_SLAB * sizeof(double) : 0;
    return orb_kat_run("orbfe_pnp_kat", in, in_b, out, out_b, ws_b, [&](void *d_in, void *d_out, void *d_ws) {
        const unsigned T = 64, B = (unsigned)((n + T - 1) / T);
        if (pose)
            k_pnp_kat_pose<<<1, 64>>>(n, (const double *)d_in, (double *)d_out, (double *)d_ws);
        else
            k_pnp_kat<<<B, T>>>(what, n, (const double *)d_in, (double *)d_out);
    });
}
