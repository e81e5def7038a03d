// orbfe_sim3.hip -- the reference's Sim3Solver (src/Sim3Solver.cc: Horn's closed form on three point pairs inside a RANSAC
// loop) on the GPU, one solver or a batch.  Every step restates tests/sim3_oracle.py operation for operation: float where the
// C++ uses float, double where it uses double, no FMA (-ffp-contract=off), sums in the C++ order; atan2 / sin / cos are the
// canonical fp64 sequences of the oracle (fdlibm's polynomials, Cody-Waite reduction), not the device library's.  So the model,
// the masks and every tap are bit-exact against the oracle's canonical mode.  Layout: DESIGN.md section 8e.
//   k_sim3_ransac   one workgroup per set.  A chunk is up to SM_K iterations: lane h takes its three draws, picks its triple
//                   (an iteration's triple depends on its own draws only) and fits one hypothesis (4x4 float Jacobi in LDS);
//                   the workgroup counts every hypothesis's inliers, points across lanes, one ballot per hypothesis and wave;
//                   lane 0 replays the acceptance rule in iteration order and stops at the first return.  The best mask is
//                   recomputed from the best model.
//   k_sim3_prepare  the constructor's Rcw * Xw + tcw for both keyframes.
// The handle, its taps and the host form's round trip are csrc/orbfe_ransac.h; here are the solver's own arrays, the argument
// checks and the kernels.
#include <float.h>
#include <math.h>

#include "orbfe_common.h"
#include "orbfe_ransac.h"
#include "orbfe_jacobi.h"
#include "orbfe_ctrig.h"

namespace {

constexpr int SM_K = 32;    // hypotheses per chunk (one lane each; 36 floats of Jacobi workspace + 34 of model in LDS per hypothesis)
constexpr int SM_T = 256;   // k_sim3_ransac workgroup
constexpr int SM_MAX_ITERATIONS = 1 << 20;

// canonical atan2 / sin / cos (tests/sim3_oracle.py c_atan2, c_sin, c_cos): csrc/orbfe_ctrig.h

// ---- ComputeSim3 ---------------------------------------------------------------------------------------------------------------
struct SmHyp {
    float R[9], s;
    float T12[12], T21[12];   // the upper three rows, [sR | t] and [sRinv | tinv]
};

// ComputeCentroid: P row-major 3x3, one point per column (oracle S1)
__device__ inline void centroid3(const float *P, float *Pr, float *O)
{
    const float third = (float)(1.0 / 3.0);
    for (int k = 0; k < 3; k++) {
        O[k] = ((P[3 * k] + P[3 * k + 2]) + P[3 * k + 1]) * third + 0.0f;
        for (int j = 0; j < 3; j++) Pr[3 * k + j] = P[3 * k + j] - O[k];
    }
}

// eigen -> quaternion -> angle-axis -> cv::Rodrigues (oracle S4-S7); A holds the N matrix, element e at A[e * st]
__device__ void rotation_from_n(float *A, float *W, float *V, int st, float *R)
{
    jacobi<4>(A, W, V, st);
    float vec[3] = {V[1 * st], V[2 * st], V[3 * st]};
    const double v0 = vec[0], v1 = vec[1], v2 = vec[2];
    const double nrm = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    const double ang = c_atan2(nrm, (double)V[0]);
    const float af = (float)((2.0 * ang) * (1.0 / nrm));
    for (int i = 0; i < 3; i++) vec[i] = vec[i] * af + 0.0f;
    const double rx = vec[0], ry = vec[1], rz = vec[2];
    const double theta = sqrt(rx * rx + ry * ry + rz * rz);
    if (theta < DBL_EPSILON) {
        for (int e = 0; e < 9; e++) R[e] = e % 4 == 0 ? 1.0f : 0.0f;
        return;
    }
    const double c = c_cos(theta), s = c_sin(theta), c1 = 1.0 - c, it = 1.0 / theta;
    const double r[3] = {rx * it, ry * it, rz * it};
    const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double rxm[9] = {0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = (float)((c * eye[3 * i + j] + c1 * (r[i] * r[j])) + s * rxm[3 * i + j]);
}

// ComputeSim3 on the triple's points (P1 / P2 row-major 3x3, one point per column)
__device__ void compute_sim3(const float *P1, const float *P2, bool fix_scale, float *A, float *W, float *V, int st, SmHyp &H)
{
    float Pr1[9], Pr2[9], O1[3], O2[3], M[9];
    centroid3(P1, Pr1, O1);
    centroid3(P2, Pr2, O2);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M[3 * i + j] = (Pr2[3 * i] * Pr1[3 * j] + Pr2[3 * i + 1] * Pr1[3 * j + 1]) + Pr2[3 * i + 2] * Pr1[3 * j + 2];
    const double m00 = M[0], m01 = M[1], m02 = M[2], m10 = M[3], m11 = M[4], m12 = M[5], m20 = M[6], m21 = M[7], m22 = M[8];
    const float N11 = (float)(m00 + m11 + m22), N12 = (float)(m12 - m21), N13 = (float)(m20 - m02), N14 = (float)(m01 - m10),
                N22 = (float)(m00 - m11 - m22), N23 = (float)(m01 + m10), N24 = (float)(m20 + m02), N33 = (float)(-m00 + m11 - m22),
                N34 = (float)(m12 + m21), N44 = (float)(-m00 - m11 + m22);
    const float Nm[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
    for (int e = 0; e < 16; e++) A[e * st] = Nm[e];
    float *R = H.R;
    rotation_from_n(A, W, V, st, R);
    float P3[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) P3[3 * i + j] = (R[3 * i] * Pr2[j] + R[3 * i + 1] * Pr2[3 + j]) + R[3 * i + 2] * Pr2[6 + j];
    float s = 1.0f;
    if (!fix_scale) {
        double nom = 0;
        for (int i = 0; i < 8; i += 4)
            nom += (((double)Pr1[i] * P3[i] + (double)Pr1[i + 1] * P3[i + 1]) + (double)Pr1[i + 2] * P3[i + 2]) + (double)Pr1[i + 3] * P3[i + 3];
        nom += (double)Pr1[8] * P3[8];
        double den = 0;
        for (int e = 0; e < 9; e++) den += (double)(P3[e] * P3[e]);
        s = (float)(nom / den);
    }
    H.s = s;
    float sR[9], t[3];
    for (int e = 0; e < 9; e++) sR[e] = R[e] * s + 0.0f;
    for (int k = 0; k < 3; k++) t[k] = O1[k] - ((sR[3 * k] * O2[0] + sR[3 * k + 1] * O2[1]) + sR[3 * k + 2] * O2[2]);
    const float ainv = (float)(1.0 / (double)s);
    float sRi[9], ti[3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) sRi[3 * i + j] = R[3 * j + i] * ainv + 0.0f;
    for (int k = 0; k < 3; k++) ti[k] = -((sRi[3 * k] * t[0] + sRi[3 * k + 1] * t[1]) + sRi[3 * k + 2] * t[2]);
    for (int k = 0; k < 3; k++) {
        for (int j = 0; j < 3; j++) {
            H.T12[4 * k + j] = sR[3 * k + j];
            H.T21[4 * k + j] = sRi[3 * k + j];
        }
        H.T12[4 * k + 3] = t[k];
        H.T21[4 * k + 3] = ti[k];
    }
}

// ---- draws, projection ---------------------------------------------------------------------------------------------------------
// the three swap-with-back / pop-back selections out of 0 .. n-1 (n >= 3) without the list: after the first removal position
// p0 holds n-1; after the second, position p1 holds what position n-2 held
__device__ inline void triple_from_draws(const int32_t *d, int n, int *tri)
{
    const int p0 = index_from_draw(d[0], n);
    tri[0] = p0;
    const int p1 = index_from_draw(d[1], n - 1);
    tri[1] = p1 == p0 ? n - 1 : p1;
    const int back = n - 2 == p0 ? n - 1 : n - 2;
    const int p2 = index_from_draw(d[2], n - 2);
    tri[2] = p2 == p1 ? back : p2 == p0 ? n - 1 : p2;
}

// Project / FromCameraToImage: K = (fx, fy, cx, cy)
__device__ inline void to_image(float x, float y, float z, const float *K, float &u, float &v)
{
    const float invz = 1.0f / z;
    const float xn = x * invz, yn = y * invz;
    u = K[0] * xn + K[2];
    v = K[1] * yn + K[3];
}

__device__ inline void project(const float *T, const float *X, const float *K, float &u, float &v)
{
    float c[3];
    for (int k = 0; k < 3; k++) c[k] = ((T[4 * k] * X[0] + T[4 * k + 1] * X[1]) + T[4 * k + 2] * X[2]) + T[4 * k + 3];
    to_image(c[0], c[1], c[2], K, u, v);
}

struct SmPoint {
    float X1[3], X2[3], p1[2], p2[2], thr1, thr2;
};

__device__ inline float max_error(float sigma2) { return (float)(unsigned long long)(9.210 * (double)sigma2); }

__device__ inline void load_point(const float *X1, const float *X2, const float *s1, const float *s2, int i, const float *K1,
                                  const float *K2, SmPoint &p)
{
    for (int k = 0; k < 3; k++) p.X1[k] = X1[3 * (size_t)i + k], p.X2[k] = X2[3 * (size_t)i + k];
    to_image(p.X1[0], p.X1[1], p.X1[2], K1, p.p1[0], p.p1[1]);
    to_image(p.X2[0], p.X2[1], p.X2[2], K2, p.p2[0], p.p2[1]);
    p.thr1 = max_error(s1[i]);
    p.thr2 = max_error(s2[i]);
}

// CheckInliers for one point
__device__ inline bool check_point(const SmPoint &p, const float *T12, const float *T21, const float *K1, const float *K2, float &e1,
                                   float &e2)
{
    float u, v;
    project(T12, p.X2, K1, u, v);
    const float a0 = p.p1[0] - u, a1 = p.p1[1] - v;
    project(T21, p.X1, K2, u, v);
    const float b0 = u - p.p2[0], b1 = v - p.p2[1];
    e1 = (float)((double)a0 * a0 + (double)a1 * a1);
    e2 = (float)((double)b0 * b0 + (double)b1 * b1);
    return e1 < p.thr1 && e2 < p.thr2;
}

struct SmArgs {
    const int32_t *off;
    const float *X1, *X2, *sig1, *sig2;
    const orbfe_sim3_set *sets;
    const int32_t *draws;
    orbfe_sim3_state *state;
    uint8_t *best_mask;
    orbfe_sim3_result *result;
    uint8_t *mask;
    const int32_t *idx1;
    uint8_t *key_mask;
    int max_points;              // bounds one set
    orbfe_sim3_iter *tap_iter;   // [tap_sets][ORBFE_SIM3_TAP_ITERS]
    float *tap_err;              // [tap_sets][max_points][2]
    int32_t *tap_info;           // [tap_sets][2]: iterations run, pairs of the set
    int tap_sets, tap_iteration;
};

__device__ inline void copy_model(orbfe_sim3_model &m, const SmHyp &h)
{
    for (int e = 0; e < 12; e++) m.T12[e] = h.T12[e];
    m.T12[12] = m.T12[13] = m.T12[14] = 0.0f;
    m.T12[15] = 1.0f;
    for (int e = 0; e < 9; e++) m.R[e] = h.R[e];
    for (int k = 0; k < 3; k++) m.t[k] = h.T12[4 * k + 3];
    m.s = h.s;
    m.reserved[0] = m.reserved[1] = m.reserved[2] = 0.0f;
}

// ---- RANSAC --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SM_T) void k_sim3_ransac(SmArgs a)
{
    __shared__ float sA[16 * SM_K], sV[16 * SM_K], sW[4 * SM_K];
    __shared__ SmHyp sH[SM_K], sBest;
    __shared__ int sTri[SM_K][3], sCnt[SM_K];
    __shared__ int sDone, sFound, sChanged, sIters, sBestInl, sRun;
    const int set = blockIdx.x, tid = threadIdx.x;
    const int o = a.off[set], n = a.off[set + 1] - o;
    const orbfe_sim3_set P = a.sets[set];
    const bool tapped = set < a.tap_sets;
    orbfe_sim3_result *res = a.result + set;
    if (tapped && tid == 0) {
        a.tap_info[2 * set] = 0;
        a.tap_info[2 * set + 1] = 0;
    }
    if (n < 0 || n > a.max_points) {   // nothing but these four words is written
        if (tid == 0) {
            res->found = 0;
            res->no_more = 1;
            res->n_inliers = 0;
            res->iterations_run = 0;
        }
        return;
    }
    orbfe_sim3_state *state = a.state + set;
    uint8_t *mask = a.mask + o, *best_mask = a.best_mask + o;
    uint8_t *key_mask = a.key_mask && P.n_keys > 0 ? a.key_mask + P.key_offset : nullptr;
    // vbInliers = vector<bool>(mN1, false)
    for (int i = tid; i < n; i += SM_T) mask[i] = 0;
    if (key_mask)
        for (int i = tid; i < P.n_keys; i += SM_T) key_mask[i] = 0;
    if (n < P.min_inliers || n < 3) {
        if (tid == 0) {
            res->found = 0;
            res->no_more = 1;
            res->n_inliers = 0;
            res->iterations_run = 0;
            res->model = state->best;
            for (int e = 0; e < 16; e++) res->model.T12[e] = 0.0f;
        }
        return;
    }
    const float *X1 = a.X1 + 3 * (size_t)o, *X2 = a.X2 + 3 * (size_t)o, *sig1 = a.sig1 + o, *sig2 = a.sig2 + o;
    if (tid == 0) {
        sIters = state->iterations;
        sBestInl = state->best_inliers;
        sDone = 0;
        sFound = 0;
        sChanged = 0;
        sRun = 0;
    }
    __syncthreads();
    for (int base = 0;; base += SM_K) {
        // the iterations of this chunk: what the call still asks for and what the clamp leaves
        const int cnt = min(SM_K, min(P.n_iterations - base, P.max_its - sIters));
        if (cnt <= 0) break;
        if (tid < cnt) {
            int tri[3];
            triple_from_draws(a.draws + P.draws_offset + 3 * (size_t)(base + tid), n, tri);
            float P1[9], P2[9];
            for (int j = 0; j < 3; j++)
                for (int k = 0; k < 3; k++) {
                    P1[3 * k + j] = X1[3 * (size_t)tri[j] + k];
                    P2[3 * k + j] = X2[3 * (size_t)tri[j] + k];
                }
            compute_sim3(P1, P2, P.fix_scale != 0, sA + tid, sW + tid, sV + tid, SM_K, sH[tid]);
            for (int j = 0; j < 3; j++) sTri[tid][j] = tri[j];
            sCnt[tid] = 0;
        }
        __syncthreads();
        // inlier counts: integer sums, any order
        for (int i0 = 0; i0 < n; i0 += SM_T) {
            const int i = i0 + tid;
            const bool valid = i < n;
            SmPoint p;
            if (valid) load_point(X1, X2, sig1, sig2, i, P.K1, P.K2, p);
            for (int h = 0; h < cnt; h++) {
                float e1 = 0, e2 = 0;
                const bool in = valid && check_point(p, sH[h].T12, sH[h].T21, P.K1, P.K2, e1, e2);
                const unsigned long long b = __ballot(in);
                if ((tid & 63) == 0 && b) atomicAdd(&sCnt[h], __popcll(b));
                if (tapped && valid && base + h == a.tap_iteration) {
                    float *te = a.tap_err + ((size_t)set * a.max_points + i) * 2;
                    te[0] = e1;
                    te[1] = e2;
                }
            }
        }
        __syncthreads();
        if (tapped && tid < cnt && base + tid < ORBFE_SIM3_TAP_ITERS) {
            orbfe_sim3_iter *ti = a.tap_iter + (size_t)set * ORBFE_SIM3_TAP_ITERS + base + tid;
            for (int j = 0; j < 3; j++) ti->triple[j] = sTri[tid][j];
            ti->n_inliers = sCnt[tid];
            for (int e = 0; e < 12; e++) ti->T12[e] = sH[tid].T12[e];
            ti->T12[12] = ti->T12[13] = ti->T12[14] = 0.0f;
            ti->T12[15] = 1.0f;
        }
        // lane 0: the serial loop over the chunk
        if (tid == 0) {
            for (int h = 0; h < cnt; h++) {
                sIters++;
                sRun++;
                const int c = sCnt[h];
                if (c >= sBestInl) {
                    sBest = sH[h];
                    sBestInl = c;
                    sChanged = 1;
                    if (c > P.min_inliers) {
                        sFound = 1;
                        sDone = 1;
                        break;
                    }
                }
            }
        }
        __syncthreads();
        if (sDone) break;
    }
    // mvbBestInliers of a best model this call set, from the model; on a return it is vbInliers too
    if (sChanged) {
        for (int i = tid; i < n; i += SM_T) {
            SmPoint p;
            load_point(X1, X2, sig1, sig2, i, P.K1, P.K2, p);
            float e1, e2;
            const bool in = check_point(p, sBest.T12, sBest.T21, P.K1, P.K2, e1, e2);
            best_mask[i] = in;
            if (sFound) {
                mask[i] = in;
                if (in && key_mask && a.idx1) {
                    const int k = a.idx1[o + i];
                    if (k >= 0 && k < P.n_keys) key_mask[k] = 1;
                }
            }
        }
    }
    if (tid == 0) {
        state->iterations = sIters;
        state->best_inliers = sBestInl;
        if (sChanged) copy_model(state->best, sBest);
        res->found = sFound;
        res->no_more = !sFound && sIters >= P.max_its;
        res->n_inliers = sFound ? sBestInl : 0;
        res->iterations_run = sRun;
        res->model = state->best;
        if (!sFound)
            for (int e = 0; e < 16; e++) res->model.T12[e] = 0.0f;
        if (tapped) {
            a.tap_info[2 * set] = sRun;
            a.tap_info[2 * set + 1] = n;
        }
    }
}

// mvX3Dc1 / mvX3Dc2: Rcw * Xw + tcw, float, left to right
struct SmPose {
    float R[9], t[3];
};

__global__ void k_sim3_prepare(int n, const float *W1, const float *W2, SmPose p1, SmPose p2, float *X1, float *X2)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int k = 0; k < 3; k++) {
        const float *a = W1 + 3 * (size_t)i, *b = W2 + 3 * (size_t)i;
        X1[3 * (size_t)i + k] = ((p1.R[3 * k] * a[0] + p1.R[3 * k + 1] * a[1]) + p1.R[3 * k + 2] * a[2]) + p1.t[k];
        X2[3 * (size_t)i + k] = ((p2.R[3 * k] * b[0] + p2.R[3 * k + 1] * b[1]) + p2.R[3 * k + 2] * b[2]) + p2.t[k];
    }
}

// ---- known-answer kernels ------------------------------------------------------------------------------------------------------
__global__ void k_sim3_kat_jacobi4(int n, float *A, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) jacobi<4>(A + (size_t)i * 16, out + (size_t)i * 20, out + (size_t)i * 20 + 4, 1);
}

__global__ void k_sim3_kat_trig(int what, int n, const double *in, double *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = what == ORBFE_SIM3_KAT_ATAN2 ? c_atan2(in[2 * i], in[2 * i + 1]) : what == ORBFE_SIM3_KAT_SIN ? c_sin(in[i]) : c_cos(in[i]);
}

__global__ void k_sim3_kat_rotation(int n, float *A, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float W[4], V[16], R[9];
    rotation_from_n(A + (size_t)i * 16, W, V, 1, R);
    for (int e = 0; e < 9; e++) out[(size_t)i * 9 + e] = R[e];
}

}  // namespace

struct orbfe_sim3 : RansacHandle {   // max_points is the create call's max_pairs
    float *d_X1 = nullptr, *d_X2 = nullptr, *d_sig1 = nullptr, *d_sig2 = nullptr;
    std::vector<OrbAlloc> blocks(size_t np) { return {orb_blk(&d_X1, np * 12), orb_blk(&d_X2, np * 12), orb_blk(&d_sig1, np * 4), orb_blk(&d_sig2, np * 4)}; }
};

static const RansacSizes SM_SIZES = {sizeof(orbfe_sim3_set), sizeof(orbfe_sim3_state), sizeof(orbfe_sim3_result), sizeof(orbfe_sim3_iter), 2,
                                     ORBFE_SIM3_TAP_SETS, ORBFE_SIM3_TAP_ITERS};

extern "C" orbfe_status orbfe_sim3_create(int32_t device, int32_t max_pairs, int32_t max_sets, orbfe_sim3 **out)
{
    return ransac_create("orbfe_sim3_create", SM_SIZES, device, max_pairs, max_sets, out);
}

extern "C" void orbfe_sim3_destroy(orbfe_sim3 *h) { orb_destroy(h, ransac_free<orbfe_sim3>); }

extern "C" void *orbfe_sim3_get_stream(orbfe_sim3 *h) { return h ? (void *)h->stream : nullptr; }

extern "C" int32_t orbfe_sim3_ransac_iterations(double probability, int32_t min_inliers, int32_t max_its, int32_t n)
{
    if (n <= 0) return 1;
    const float epsilon = (float)min_inliers / (float)n;
    int32_t its = min_inliers == n ? 1 : x86_double_to_int(ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3))));
    if (its > max_its) its = max_its;
    return its < 1 ? 1 : its;
}

static orbfe_status sim3_launch(orbfe_sim3 *h, SmArgs &a, int nsets, hipStream_t st)
{
    ransac_bind_taps(h, a, nsets, st);
    if (nsets == 0) return ORBFE_OK;
    k_sim3_ransac<<<nsets, SM_T, 0, st>>>(a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_sim3_iterate(orbfe_sim3 *h, const float *X1, const float *X2, const float *sigma2_1, const float *sigma2_2,
                                           int32_t n, const float *K1, const float *K2, int32_t fix_scale, int32_t min_inliers,
                                           int32_t max_its, int32_t n_iterations, const int32_t *draws, orbfe_sim3_state *state,
                                           uint8_t *best_mask, orbfe_sim3_result *result, uint8_t *mask)
{
    if (!h || !K1 || !K2 || !state || !result || n < 0 || (n > 0 && (!X1 || !X2 || !sigma2_1 || !sigma2_2 || !best_mask))) {
        orbfe_set_error("orbfe_sim3_iterate: a required pointer is NULL or n < 0");
        return ORBFE_ERR_ARG;
    }
    if (n > h->max_points) {
        orbfe_set_error("%d pairs exceed max_pairs %d", n, h->max_points);
        return ORBFE_ERR_ARG;
    }
    if (n_iterations < 0 || n_iterations > SM_MAX_ITERATIONS || (n_iterations > 0 && !draws)) {
        orbfe_set_error("n_iterations %d outside [0, %d], or no draws", n_iterations, SM_MAX_ITERATIONS);
        return ORBFE_ERR_ARG;
    }
    if (min_inliers < 0 || state->iterations < 0 || state->best_inliers < 0) {
        orbfe_set_error("negative min_inliers or state counters");
        return ORBFE_ERR_ARG;
    }
    DeviceGuard dg(h->device);
    orbfe_sim3_set set = {};
    for (int k = 0; k < 4; k++) set.K1[k] = K1[k], set.K2[k] = K2[k];
    set.fix_scale = fix_scale != 0;
    set.min_inliers = min_inliers;
    set.max_its = max_its;
    set.n_iterations = n_iterations;
    SmArgs a = {};
    a.X1 = h->d_X1;
    a.X2 = h->d_X2;
    a.sig1 = h->d_sig1;
    a.sig2 = h->d_sig2;
    return ransac_host_call(h, SM_SIZES, a, sim3_launch, n, &set, state, draws, 3 * (size_t)n_iterations,
                            {{h->d_X1, X1, 12}, {h->d_X2, X2, 12}, {h->d_sig1, sigma2_1, 4}, {h->d_sig2, sigma2_2, 4}}, best_mask, result, mask);
}

extern "C" orbfe_status orbfe_sim3_iterate_device(orbfe_sim3 *h, const int32_t *d_offsets, const float *d_X1, const float *d_X2,
                                                  const float *d_sigma2_1, const float *d_sigma2_2, const orbfe_sim3_set *d_sets,
                                                  const int32_t *d_draws, int32_t nsets, orbfe_sim3_state *d_state, uint8_t *d_best_mask,
                                                  orbfe_sim3_result *d_result, uint8_t *d_mask, const int32_t *d_idx1, uint8_t *d_key_mask,
                                                  void *stream)
{
    if (!h || nsets < 0 ||
        (nsets > 0 && (!d_offsets || !d_X1 || !d_X2 || !d_sigma2_1 || !d_sigma2_2 || !d_sets || !d_draws || !d_state || !d_best_mask ||
                       !d_result || !d_mask))) {
        orbfe_set_error("orbfe_sim3_iterate_device: a required pointer is NULL or nsets < 0");
        return ORBFE_ERR_ARG;
    }
    if ((d_idx1 == nullptr) != (d_key_mask == nullptr)) {
        orbfe_set_error("d_idx1 and d_key_mask go together");
        return ORBFE_ERR_ARG;
    }
    if (nsets > h->max_sets) {
        orbfe_set_error("%d sets exceed max_sets %d", nsets, h->max_sets);
        return ORBFE_ERR_ARG;
    }
    DeviceGuard dg(h->device);
    SmArgs a = {};
    a.off = d_offsets;
    a.X1 = d_X1;
    a.X2 = d_X2;
    a.sig1 = d_sigma2_1;
    a.sig2 = d_sigma2_2;
    a.sets = d_sets;
    a.draws = d_draws;
    a.state = d_state;
    a.best_mask = d_best_mask;
    a.result = d_result;
    a.mask = d_mask;
    a.idx1 = d_idx1;
    a.key_mask = d_key_mask;
    return sim3_launch(h, a, nsets, (hipStream_t)stream);
}

extern "C" orbfe_status orbfe_sim3_prepare_device(orbfe_sim3 *h, const float *d_world1, const float *d_world2, int32_t n,
                                                  const float *Rcw1, const float *tcw1, const float *Rcw2, const float *tcw2, float *d_X1,
                                                  float *d_X2, void *stream)
{
    if (!h || n < 0 || !Rcw1 || !tcw1 || !Rcw2 || !tcw2 || (n > 0 && (!d_world1 || !d_world2 || !d_X1 || !d_X2))) {
        orbfe_set_error("orbfe_sim3_prepare_device: a required pointer is NULL or n < 0");
        return ORBFE_ERR_ARG;
    }
    if (n == 0) return ORBFE_OK;
    SmPose p1, p2;
    for (int e = 0; e < 9; e++) p1.R[e] = Rcw1[e], p2.R[e] = Rcw2[e];
    for (int e = 0; e < 3; e++) p1.t[e] = tcw1[e], p2.t[e] = tcw2[e];
    DeviceGuard dg(h->device);
    k_sim3_prepare<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(n, d_world1, d_world2, p1, p2, d_X1, d_X2);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_sim3_set_tap_iteration(orbfe_sim3 *h, int32_t iteration)
{
    return ransac_set_tap_iteration(h, SM_SIZES, "orbfe_sim3_set_tap_iteration", iteration);
}

extern "C" orbfe_status orbfe_sim3_tap(orbfe_sim3 *h, int32_t set, int32_t stage, void *dst, size_t cap, int32_t *count)
{
    if (!h || !dst || !count || stage < ORBFE_SIM3_TAP_ITERATIONS || stage > ORBFE_SIM3_TAP_ERRORS) return ORBFE_ERR_ARG;
    return ransac_tap(h, SM_SIZES, set, stage == ORBFE_SIM3_TAP_ITERATIONS, dst, cap, count);
}

extern "C" orbfe_status orbfe_sim3_kat(int32_t what, int32_t n, const void *in, void *out)
{
    if (n < 0 || !out || (!in && n > 0) || what < ORBFE_SIM3_KAT_JACOBI4 || what > ORBFE_SIM3_KAT_ROTATION) return ORBFE_ERR_ARG;
    if (n == 0) return ORBFE_OK;
    size_t in_b = 0, out_b = 0;
    switch (what) {
    case ORBFE_SIM3_KAT_JACOBI4: in_b = (size_t)n * 64; out_b = (size_t)n * 80; break;
    case ORBFE_SIM3_KAT_ATAN2: in_b = (size_t)n * 16; out_b = (size_t)n * 8; break;
    case ORBFE_SIM3_KAT_ROTATION: in_b = (size_t)n * 64; out_b = (size_t)n * 36; break;
    default: in_b = (size_t)n * 8; out_b = (size_t)n * 8; break;
    }
    return orb_kat_run("orbfe_sim3_kat", in, in_b, out, out_b, 0, [&](void *d_in, void *d_out, void *) {
        const unsigned T = 128, B = (unsigned)((n + T - 1) / T);
        switch (what) {
        case ORBFE_SIM3_KAT_JACOBI4: k_sim3_kat_jacobi4<<<B, T>>>(n, (float *)d_in, (float *)d_out); break;
        case ORBFE_SIM3_KAT_ROTATION: k_sim3_kat_rotation<<<B, T>>>(n, (float *)d_in, (float *)d_out); break;
        default: k_sim3_kat_trig<<<B, T>>>(what, n, (const double *)d_in, (double *)d_out); break;
        }
    });
}
