// orbfe_bow.hip -- the bag-of-words side of the matcher handle (include/orbfe.h "Matcher"): SearchByBoW, the vocabulary and the BoW
// transform, their device-resident batched chain, and MapPoint::ComputeDistinctiveDescriptors.
#include <algorithm>
#include <new>
#include <vector>

#include "orbfe_common.h"
#include "orbfe_matcher.h"
#include "orbfe_match_dev.h"

// ---------------------------------------------------------------------------------------------------
// K9  SearchByBoW: one thread per KeyFrame vocabulary node.  Nodes own disjoint feature sets, so the
// greedy "F feature already claimed" rule (:273-274, :725) only couples features inside one node and
// is replayed serially there, in the reference's iteration order.
// matchF2KF[iF] = KF feature index, -1 none.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_search_by_bow(const uint8_t *__restrict__ descKF,
                                                      const uint8_t *__restrict__ validKF,
                                                      const uint32_t *__restrict__ nodeKF,
                                                      const uint32_t *__restrict__ offKF,
                                                      const uint32_t *__restrict__ idxKF, int nnodesKF,
                                                      const uint8_t *__restrict__ descF,
                                                      const uint8_t *__restrict__ validF,
                                                      const uint32_t *__restrict__ nodeF,
                                                      const uint32_t *__restrict__ offF,
                                                      const uint32_t *__restrict__ idxF, int nnodesF, float nnratio,
                                                      int th_low, int strict_lt, int32_t *__restrict__ matchF2KF)
{
    const int a = blockIdx.x * 64 + threadIdx.x;
    if (a >= nnodesKF) return;
    const uint32_t node = nodeKF[a];
    int lo = 0, hi = nnodesF - 1, b = -1;  // lower_bound walk of :329-333 == binary search on sorted ids
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const uint32_t v = nodeF[mid];
        if (v == node) { b = mid; break; }
        if (v < node) lo = mid + 1; else hi = mid - 1;
    }
    if (b < 0) return;
    for (uint32_t ik = offKF[a]; ik < offKF[a + 1]; ++ik) {
        const uint32_t rk = idxKF[ik];
        if (validKF && !validKF[rk]) continue;
        const Desc8 dk = load_desc8(descKF + (int64_t)rk * 32);
        int b1 = 256, b2 = 256, bi = -1;
        for (uint32_t jf = offF[b]; jf < offF[b + 1]; ++jf) {
            const uint32_t rf = idxF[jf];
            if (matchF2KF[rf] >= 0) continue;
            if (validF && !validF[rf]) continue;
            const int d = hamming8(dk, (const uint32_t *)(descF + (int64_t)rf * 32));
            if (d < b1) { b2 = b1; b1 = d; bi = (int)rf; }
            else if (d < b2) { b2 = d; }
        }
        const bool pass = strict_lt ? (b1 < th_low) : (b1 <= th_low);
        if (pass && bi >= 0 && (float)b1 < __fmul_rn(nnratio, (float)b2)) matchF2KF[bi] = (int32_t)rk;
    }
}

// rotation prune for SearchByBoW: key = F feature i, rot = angKF[match[i]] - angF[i] (:308, :759)
__global__ __launch_bounds__(256) void k_rot_prune_bow(int32_t *__restrict__ match, const float *__restrict__ angKF,
                                                       const float *__restrict__ angF, int nF, int check_ori,
                                                       int32_t *__restrict__ nmatches)
{
    rot_prune(match, nF, check_ori, nmatches, [&](int, int j) { return angKF[j]; }, [&](int i, int) { return angF[i]; });
}

static bool csr_ok(const uint32_t *node, const uint32_t *off, const uint32_t *idx, int nn, int nfeat,
                   std::vector<uint8_t> &seen)
{
    seen.assign((size_t)std::max(nfeat, 1), 0);
    for (int a = 0; a < nn; ++a) {
        if (a > 0 && node[a] <= node[a - 1]) return false;
        if (off[a + 1] < off[a]) return false;
        for (uint32_t k = off[a]; k < off[a + 1]; ++k) {
            if (idx[k] >= (uint32_t)nfeat || seen[idx[k]]) return false;
            seen[idx[k]] = 1;
        }
    }
    return true;
}

extern "C" orbfe_status orbfe_search_by_bow(orbfe_matcher *m, const uint8_t *descKF, int32_t nKF,
                                            const uint8_t *validKF, const float *angKF, const uint32_t *nodeKF,
                                            const uint32_t *offKF, const uint32_t *idxKF, int32_t nnodesKF,
                                            const uint8_t *descF, int32_t nF, const uint8_t *validF,
                                            const float *angF, const uint32_t *nodeF, const uint32_t *offF,
                                            const uint32_t *idxF, int32_t nnodesF, float nnratio, int32_t th_low,
                                            int32_t strict_lt, int32_t check_ori, int32_t *matchF2KF,
                                            int32_t *nmatches)
{
    if (!m || nKF < 0 || nF < 0 || nnodesKF < 0 || nnodesF < 0 || (nF > 0 && !matchF2KF) ||
        (nnodesKF > 0 && (!nodeKF || !offKF || !descKF)) || (nnodesF > 0 && (!nodeF || !offF || !descF)) ||
        (check_ori && (nKF > 0 && nF > 0) && (!angKF || !angF))) {
        orbfe_set_error("bad argument to orbfe_search_by_bow");
        return ORBFE_ERR_ARG;
    }
    for (int i = 0; i < nF; ++i) matchF2KF[i] = -1;
    if (nmatches) *nmatches = 0;
    if (nKF == 0 || nF == 0 || nnodesKF == 0 || nnodesF == 0) return ORBFE_OK;
    std::vector<uint8_t> seen;
    if (!csr_ok(nodeKF, offKF, idxKF, nnodesKF, nKF, seen) || !csr_ok(nodeF, offF, idxF, nnodesF, nF, seen)) {
        orbfe_set_error("feature vector CSR invalid: node ids must ascend, indices in range and unique");
        return ORBFE_ERR_ARG;
    }
    DeviceGuard g(m->device);
    hipStream_t st = m->stream;
    ORBFE_HIP(scratch_acquire(m, st));  // a device-buffer call on another stream may still be using the scratch blocks
    const size_t nikf = offKF[nnodesKF], nif = offF[nnodesF];
    const size_t sz[14] = {(size_t)nKF * 32, (size_t)nKF, (size_t)nKF * 4, (size_t)nnodesKF * 4,
                           (size_t)(nnodesKF + 1) * 4, nikf * 4, (size_t)nF * 32, (size_t)nF, (size_t)nF * 4,
                           (size_t)nnodesF * 4, (size_t)(nnodesF + 1) * 4, nif * 4, (size_t)nF * 4, 4};
    const void *src[12] = {descKF, validKF, angKF, nodeKF, offKF, idxKF, descF, validF, angF, nodeF, offF, idxF};
    for (int i = 0; i < 14; ++i) ORBFE_HIP(m->b[i].ensure(sz[i]));
    for (int i = 0; i < 12; ++i)
        if (src[i] && sz[i]) ORBFE_HIP(hipMemcpyAsync(m->b[i].p, src[i], sz[i], hipMemcpyHostToDevice, st));
    ORBFE_HIP(hipMemsetAsync(m->b[12].p, 0xFF, (size_t)nF * 4, st));
    hipLaunchKernelGGL(k_search_by_bow, dim3((nnodesKF + 63) / 64), dim3(64), 0, st, m->b[0].as<const uint8_t>(),
                       validKF ? m->b[1].as<const uint8_t>() : nullptr, m->b[3].as<const uint32_t>(),
                       m->b[4].as<const uint32_t>(), m->b[5].as<const uint32_t>(), nnodesKF, m->b[6].as<const uint8_t>(),
                       validF ? m->b[7].as<const uint8_t>() : nullptr, m->b[9].as<const uint32_t>(),
                       m->b[10].as<const uint32_t>(), m->b[11].as<const uint32_t>(), nnodesF, nnratio, th_low,
                       strict_lt ? 1 : 0, m->b[12].as<int32_t>());
    ORBFE_HIP(hipGetLastError());
    // histogram key = F feature i, rot = angKF[match[i]] - angF[i] (:308, :759)
    hipLaunchKernelGGL(k_rot_prune_bow, dim3(1), dim3(256), 0, st, m->b[12].as<int32_t>(), m->b[2].as<const float>(),
                       m->b[8].as<const float>(), nF, check_ori ? 1 : 0, m->b[13].as<int32_t>());
    ORBFE_HIP(hipGetLastError());
    int32_t nm = 0;
    ORBFE_HIP(hipMemcpyAsync(matchF2KF, m->b[12].p, (size_t)nF * 4, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipMemcpyAsync(&nm, m->b[13].p, 4, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    if (nmatches) *nmatches = nm;
    return ORBFE_OK;
}

// ---------------------------------------------------------------------------------------------------
// SURVEY 8(f).3  DBoW2 TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup) as called at
// src/Frame.cc:553 and src/KeyFrame.cc:82.  DBoW2 is not vendored by the reference; the algorithm is restated from the
// published one.
// k_bow_descend: thread per feature walks the tree, per level the child with the smallest Hamming distance (first on
//   ties); remembers the node at level L - levelsup; features whose word has weight 0 are dropped.
// k_bow_aggregate: one workgroup turns the per-feature (word, node, weight) into the two containers of the reference:
//   an LDS bitonic sort by (word, feature) gives std::map order, every first-of-its-word thread adds its weights in
//   feature order (doubles, the order `+=` ran in the reference), thread 0 forms the L1 norm in ascending word order,
//   then the same sort by (node, feature) gives the FeatureVector as the CSR orbfe_search_by_bow consumes.
// ---------------------------------------------------------------------------------------------------
#define BOW_MAX_FEATURES 8192

struct orbfe_vocabulary {
    int device = 0, nnodes = 0, L = 0;
    DevBuf child_off, child_idx, node_desc, word_id, weight;
};

__global__ __launch_bounds__(256) void k_bow_descend(const uint32_t *__restrict__ child_off,
                                                     const uint32_t *__restrict__ child_idx,
                                                     const uint8_t *__restrict__ node_desc,
                                                     const uint32_t *__restrict__ word_id,
                                                     const double *__restrict__ weight, int nid_level,
                                                     const uint8_t *__restrict__ desc, int n,
                                                     int32_t *__restrict__ f_word, int32_t *__restrict__ f_node,
                                                     double *__restrict__ f_weight,
                                                     const int32_t *__restrict__ n_arr, int stride)
{
    // batched form: frame blockIdx.y owns `stride` slots of every array and holds n_arr[frame] features
    if (n_arr) {
        const int b = blockIdx.y;
        n = min(n_arr[b], stride);
        desc += (int64_t)b * stride * 32;
        f_word += (int64_t)b * stride;
        f_node += (int64_t)b * stride;
        f_weight += (int64_t)b * stride;
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (n_arr && i >= n && i < stride) {  // padding slots carry "no word" so the buffers can be used as they are
        f_word[i] = -1;
        f_node[i] = -1;
        f_weight[i] = 0.0;
    }
    if (i >= n) return;
    const Desc8 q = load_desc8(desc + (int64_t)i * 32);
    uint32_t fin = 0, nid = 0;
    int level = 0;
    uint32_t c0 = child_off[0], c1 = child_off[1];
    if (c1 == c0) {  // a root without children is DBoW2's empty() vocabulary: no feature has a word, child_idx has no entry
        f_word[i] = -1;
        f_node[i] = -1;
        f_weight[i] = 0.0;
        return;
    }
    do {  // child ids are larger than their parent's (checked at creation): the walk ends
        ++level;
        fin = child_idx[c0];
        int best = hamming8(q, (const uint32_t *)(node_desc + (int64_t)fin * 32));
        for (uint32_t c = c0 + 1; c < c1; ++c) {
            const uint32_t id = child_idx[c];
            const int d = hamming8(q, (const uint32_t *)(node_desc + (int64_t)id * 32));
            if (d < best) { best = d; fin = id; }
        }
        if (level == nid_level) nid = fin;
        c0 = child_off[fin];
        c1 = child_off[fin + 1];
    } while (c1 != c0);
    const double w = weight[fin];
    const bool keep = w > 0;
    f_word[i] = keep ? (int32_t)word_id[fin] : -1;
    f_node[i] = keep ? (int32_t)nid : -1;
    f_weight[i] = keep ? w : 0.0;
}

__device__ void bow_bitonic_sort(unsigned long long *key, int P, int tid)
{
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P; t += 1024) {
                const int ixj = t ^ j;
                if (ixj > t) {
                    const unsigned long long a = key[t], b = key[ixj];
                    const bool up = (t & k) == 0;
                    if ((a > b) == up) { key[t] = b; key[ixj] = a; }
                }
            }
            __syncthreads();
        }
}

// exclusive position of every flagged element among P (each thread owns a contiguous chunk); returns the total
__device__ int bow_positions(const unsigned long long *key, int P, int tid, int *s_scan, int *pos_of_first_in_chunk)
{
    const int chunk = (P + 1023) / 1024, j0 = tid * chunk, j1 = min(j0 + chunk, P);
    int cnt = 0;
    for (int j = j0; j < j1; ++j) {
        const unsigned long long kj = key[j];
        if (kj != ~0ull && (j == 0 || (key[j - 1] >> 32) != (kj >> 32))) ++cnt;
    }
    s_scan[tid] = cnt;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = tid >= d ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    *pos_of_first_in_chunk = s_scan[tid] - cnt;
    const int total = s_scan[1023];
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(1024) void k_bow_aggregate(int n, int P, const int32_t *__restrict__ f_word,
                                                        const int32_t *__restrict__ f_node,
                                                        const double *__restrict__ f_weight,
                                                        uint32_t *__restrict__ bow_id, double *__restrict__ bow_val,
                                                        uint32_t *__restrict__ fv_node, uint32_t *__restrict__ fv_off,
                                                        uint32_t *__restrict__ fv_idx, int32_t *__restrict__ counts,
                                                        const int32_t *__restrict__ n_arr, int stride)
{
    if (n_arr) {  // batched form: one workgroup per frame, `stride` slots per array (stride + 1 for fv_off, 4 counts)
        const int b = blockIdx.x;
        n = min(n_arr[b], stride);
        f_word += (int64_t)b * stride;
        f_node += (int64_t)b * stride;
        f_weight += (int64_t)b * stride;
        bow_id += (int64_t)b * stride;
        bow_val += (int64_t)b * stride;
        fv_node += (int64_t)b * stride;
        fv_off += (int64_t)b * (stride + 1);
        fv_idx += (int64_t)b * stride;
        counts += (int64_t)b * 4;
    }
    extern __shared__ unsigned long long s_key[];  // [P] keys, then [P] doubles
    double *s_val = (double *)(s_key + P);
    __shared__ int s_scan[1024];
    __shared__ double s_norm;
    const int tid = threadIdx.x;
    const int chunk = (P + 1023) / 1024, j0 = tid * chunk, j1 = min(j0 + chunk, P);
    // ---- BowVector ----
    for (int i = tid; i < P; i += 1024)
        s_key[i] = (i < n && f_word[i] >= 0) ? (((unsigned long long)(uint32_t)f_word[i] << 32) | (uint32_t)i) : ~0ull;
    __syncthreads();
    bow_bitonic_sort(s_key, P, tid);
    int pos;
    const int nbow = bow_positions(s_key, P, tid, s_scan, &pos);
    for (int j = j0; j < j1; ++j) {
        const unsigned long long kj = s_key[j];
        if (kj != ~0ull && (j == 0 || (s_key[j - 1] >> 32) != (kj >> 32))) {
            double v = 0.0;  // map[word] += weight, in feature order
            for (int e = j; e < P && (s_key[e] >> 32) == (kj >> 32); ++e) v = __dadd_rn(v, f_weight[(uint32_t)s_key[e]]);
            bow_id[pos] = (uint32_t)(kj >> 32);
            s_val[pos] = v;
            ++pos;
        }
    }
    __syncthreads();
    if (tid == 0) {  // BowVector::normalize(L1): ascending word order
        double norm = 0.0;
        for (int o = 0; o < nbow; ++o) norm = __dadd_rn(norm, fabs(s_val[o]));
        s_norm = norm;
    }
    __syncthreads();
    for (int o = tid; o < nbow; o += 1024) bow_val[o] = s_norm > 0.0 ? __ddiv_rn(s_val[o], s_norm) : s_val[o];
    __syncthreads();
    // ---- FeatureVector ----
    for (int i = tid; i < P; i += 1024)
        s_key[i] = (i < n && f_node[i] >= 0) ? (((unsigned long long)(uint32_t)f_node[i] << 32) | (uint32_t)i) : ~0ull;
    __syncthreads();
    bow_bitonic_sort(s_key, P, tid);
    const int nfv = bow_positions(s_key, P, tid, s_scan, &pos);
    int m = 0;
    for (int j = j0; j < j1; ++j) {
        const unsigned long long kj = s_key[j];
        if (kj == ~0ull) continue;
        fv_idx[j] = (uint32_t)kj;
        if (j == 0 || (s_key[j - 1] >> 32) != (kj >> 32)) {
            fv_node[pos] = (uint32_t)(kj >> 32);
            fv_off[pos] = (uint32_t)j;
            ++pos;
        }
        ++m;
    }
    s_scan[tid] = m;
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
        for (int t = 0; t < 1024; ++t) tot += s_scan[t];
        fv_off[nfv] = (uint32_t)tot;
        counts[0] = nbow;
        counts[1] = nfv;
        counts[2] = tot;
    }
}

extern "C" orbfe_status orbfe_vocabulary_create(int32_t device, int32_t nnodes, const uint32_t *child_off,
                                                const uint32_t *child_idx, const uint8_t *node_desc,
                                                const uint32_t *word_id, const double *weight, int32_t L,
                                                orbfe_vocabulary **out)
{
    if (!out || nnodes < 1 || !child_off || !node_desc || !word_id || !weight || L < 1) {
        orbfe_set_error("bad argument to orbfe_vocabulary_create");
        return ORBFE_ERR_ARG;
    }
    *out = nullptr;
    const uint32_t nc = child_off[nnodes];
    if (child_off[0] != 0 || (nc > 0 && !child_idx)) { orbfe_set_error("vocabulary: bad child CSR"); return ORBFE_ERR_ARG; }
    for (int i = 0; i < nnodes; ++i) {
        if (child_off[i + 1] < child_off[i]) { orbfe_set_error("vocabulary: child offsets must not decrease"); return ORBFE_ERR_ARG; }
        if (child_off[i + 1] == child_off[i] && word_id[i] > 0x7FFFFFFFu) {  // f_word is int32 and -1 means "no word"
            orbfe_set_error("vocabulary: leaf %d has word id %u, word ids must be below 2^31", i, word_id[i]);
            return ORBFE_ERR_ARG;
        }
        for (uint32_t c = child_off[i]; c < child_off[i + 1]; ++c)
            if (child_idx[c] <= (uint32_t)i || child_idx[c] >= (uint32_t)nnodes) {
                orbfe_set_error("vocabulary: child ids must be larger than their parent's id and < nnodes");
                return ORBFE_ERR_ARG;
            }
    }
    if (device < 0) device = 0;   // a vocabulary without a device argument lives on device 0, not on the current one
    const orbfe_status rs = orb_resolve_device(&device);
    if (rs != ORBFE_OK) return rs;
    orbfe_vocabulary *v = new (std::nothrow) orbfe_vocabulary();
    if (!v) return ORBFE_ERR_NOMEM;
    v->device = device;
    v->nnodes = nnodes;
    v->L = L;
    DeviceGuard g(device);
    auto up = [&](DevBuf &b, const void *src, size_t bytes) -> hipError_t {
        hipError_t e = b.ensure(std::max(bytes, (size_t)4));
        if (e == hipSuccess && bytes) e = hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice);
        return e;
    };
    hipError_t e = up(v->child_off, child_off, (size_t)(nnodes + 1) * 4);
    if (e == hipSuccess) e = up(v->child_idx, child_idx, (size_t)nc * 4);
    if (e == hipSuccess) e = up(v->node_desc, node_desc, (size_t)nnodes * 32);
    if (e == hipSuccess) e = up(v->word_id, word_id, (size_t)nnodes * 4);
    if (e == hipSuccess) e = up(v->weight, weight, (size_t)nnodes * 8);
    if (e != hipSuccess) {
        orbfe_set_error("vocabulary upload failed: %s", hipGetErrorString(e));
        orbfe_vocabulary_destroy(v);
        return ORBFE_ERR_HIP;
    }
    *out = v;
    return ORBFE_OK;
}

extern "C" void orbfe_vocabulary_destroy(orbfe_vocabulary *v)
{
    if (!v) return;
    DeviceGuard g(v->device);
    DevBuf *bufs[] = {&v->child_off, &v->child_idx, &v->node_desc, &v->word_id, &v->weight};
    for (DevBuf *b : bufs) b->release();
    delete v;
}

extern "C" orbfe_status orbfe_bow_transform(orbfe_matcher *m, const orbfe_vocabulary *v, const uint8_t *desc, int32_t n,
                                            int32_t levelsup, int32_t *f_word, int32_t *f_node, double *f_weight,
                                            uint32_t *bow_id, double *bow_val, int32_t *nbow, uint32_t *fv_node,
                                            uint32_t *fv_off, uint32_t *fv_idx, int32_t *nfv)
{
    if (!m || !v || n < 0 || n > BOW_MAX_FEATURES || !nbow || !nfv || !fv_off ||
        (n > 0 && (!desc || !bow_id || !bow_val || !fv_node || !fv_idx))) {
        orbfe_set_error("bad argument to orbfe_bow_transform (at most %d features per call)", BOW_MAX_FEATURES);
        return ORBFE_ERR_ARG;
    }
    if (v->device != m->device) { orbfe_set_error("vocabulary and matcher are on different devices"); return ORBFE_ERR_ARG; }
    *nbow = 0;
    *nfv = 0;
    fv_off[0] = 0;
    if (n == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    hipStream_t st = m->stream;
    ORBFE_HIP(scratch_acquire(m, st));  // a device-buffer call on another stream may still be using the scratch blocks
    int P = 2;
    while (P < n) P <<= 1;
    ORBFE_HIP(m->b[0].ensure((size_t)n * 32));
    ORBFE_HIP(m->b[1].ensure((size_t)n * 4));   // f_word
    ORBFE_HIP(m->b[2].ensure((size_t)n * 4));   // f_node
    ORBFE_HIP(m->b[3].ensure((size_t)n * 8));   // f_weight
    ORBFE_HIP(m->b[4].ensure((size_t)n * 4));   // bow_id
    ORBFE_HIP(m->b[5].ensure((size_t)n * 8));   // bow_val
    ORBFE_HIP(m->b[6].ensure((size_t)n * 4));   // fv_node
    ORBFE_HIP(m->b[7].ensure((size_t)(n + 1) * 4));
    ORBFE_HIP(m->b[8].ensure((size_t)n * 4));   // fv_idx
    ORBFE_HIP(m->b[9].ensure(16));
    ORBFE_HIP(hipMemcpyAsync(m->b[0].p, desc, (size_t)n * 32, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bow_descend, dim3((n + 255) / 256), dim3(256), 0, st, v->child_off.as<const uint32_t>(),
                       v->child_idx.as<const uint32_t>(), v->node_desc.as<const uint8_t>(), v->word_id.as<const uint32_t>(),
                       v->weight.as<const double>(), v->L - levelsup, m->b[0].as<const uint8_t>(), n, m->b[1].as<int32_t>(),
                       m->b[2].as<int32_t>(), m->b[3].as<double>(), (const int32_t *)nullptr, 0);
    const size_t lds = (size_t)P * 16;
    // The dynamic-LDS limit is a process-wide, per-kernel attribute: every caller sets it to the SAME value -- all of the
    // CU's LDS that the kernel's static allocation leaves -- so concurrent matchers can never lower it under one another.
    hipFuncAttributes fa;
    ORBFE_HIP(hipFuncGetAttributes(&fa, (const void *)k_bow_aggregate));
    const size_t lds_max = (size_t)ORBFE_LDS_MAX - fa.sharedSizeBytes;
    if (lds > lds_max) { orbfe_set_error("orbfe_bow_transform: %d features need more than the CU's LDS", n); return ORBFE_ERR_SIZE; }
    if (lds > 64 * 1024)
        ORBFE_HIP(hipFuncSetAttribute((const void *)k_bow_aggregate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
    hipLaunchKernelGGL(k_bow_aggregate, dim3(1), dim3(1024), lds, st, n, P, m->b[1].as<const int32_t>(),
                       m->b[2].as<const int32_t>(), m->b[3].as<const double>(), m->b[4].as<uint32_t>(), m->b[5].as<double>(),
                       m->b[6].as<uint32_t>(), m->b[7].as<uint32_t>(), m->b[8].as<uint32_t>(), m->b[9].as<int32_t>(),
                       (const int32_t *)nullptr, 0);
    ORBFE_HIP(hipGetLastError());
    int32_t counts[3] = {0, 0, 0};
    ORBFE_HIP(hipMemcpyAsync(counts, m->b[9].p, 12, hipMemcpyDeviceToHost, st));
    if (f_word) ORBFE_HIP(hipMemcpyAsync(f_word, m->b[1].p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (f_node) ORBFE_HIP(hipMemcpyAsync(f_node, m->b[2].p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (f_weight) ORBFE_HIP(hipMemcpyAsync(f_weight, m->b[3].p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    *nbow = counts[0];
    *nfv = counts[1];
    if (counts[0] > 0) {
        ORBFE_HIP(hipMemcpy(bow_id, m->b[4].p, (size_t)counts[0] * 4, hipMemcpyDeviceToHost));
        ORBFE_HIP(hipMemcpy(bow_val, m->b[5].p, (size_t)counts[0] * 8, hipMemcpyDeviceToHost));
    }
    ORBFE_HIP(hipMemcpy(fv_off, m->b[7].p, (size_t)(counts[1] + 1) * 4, hipMemcpyDeviceToHost));
    if (counts[1] > 0) ORBFE_HIP(hipMemcpy(fv_node, m->b[6].p, (size_t)counts[1] * 4, hipMemcpyDeviceToHost));
    if (counts[2] > 0) ORBFE_HIP(hipMemcpy(fv_idx, m->b[8].p, (size_t)counts[2] * 4, hipMemcpyDeviceToHost));
    return ORBFE_OK;
}

// ---------------------------------------------------------------------------------------------------
// Device-resident, batched chain behind Frame::ComputeBoW -> ORBmatcher::SearchByBoW: no host round trip between the
// extractor's output block and the matches.
//
// K9b  k_search_by_bow_rows: SIXTEEN LANES (one DPP row) per KeyFrame vocabulary node, four nodes per wave.  The F
// features of the matching node sit on the lanes; for every KF feature of the node (serial: the greedy "F feature already
// claimed" rule, :273-274 / :725, couples them) all lanes evaluate their xor / popcount distance at once and two row
// reductions (v_min over row_ror DPP moves) give best / first position / second.  Lists longer than a row are walked in
// chunks of 16 in list order, merged with the reference's "earlier position wins" rule.  Claim flags of the first chunk
// live in a register, later chunks re-read the match row (written by this very row only: nodes own disjoint features).
// ---------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ uint32_t row_ror_u32(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t row_min_u32(uint32_t v)  // minimum over the 16 lanes of the DPP row, in every lane
{
    v = min(v, row_ror_u32<0x128>(v));  // row_ror:8
    v = min(v, row_ror_u32<0x124>(v));  // row_ror:4
    v = min(v, row_ror_u32<0x122>(v));  // row_ror:2
    v = min(v, row_ror_u32<0x121>(v));  // row_ror:1
    return v;
}

struct BowBatch {
    const uint8_t *desc;        // [B][cap][32]
    const orbfe_keypoint *kps;  // [B][cap]   (angles)
    const uint8_t *valid;       // [B][cap] or null: 1 = the feature has a good MapPoint
    const uint32_t *fv_node, *fv_off, *fv_idx;  // [B][cap], [B][cap+1], [B][cap]
    const int32_t *counts;      // [B][4] {nbow, nfv, nidx, -}
    const int32_t *kf, *f;      // [P] frame indices of the pairs
    int32_t cap, npairs, th_low, strict_lt, use_valid_f, check_ori;
    float nnratio;
    int32_t *match;             // [P][cap] F feature -> KF feature, -1 none
    int32_t *nmatches;          // [P]
};

__global__ __launch_bounds__(256) void k_search_by_bow_rows(BowBatch a)
{
    __shared__ uint4 s_dk[16][16][2];
    __shared__ uint32_t s_rk[16][16];
    const int p = blockIdx.y;
    const int kf = a.kf[p], f = a.f[p];
    const int lane16 = threadIdx.x & 15, rowb = threadIdx.x >> 4;
    const int row = (blockIdx.x * 256 + threadIdx.x) >> 4, nrows = (gridDim.x * 256) >> 4;
    const int nnK = a.counts[kf * 4 + 1], nnF = a.counts[f * 4 + 1];
    const uint32_t *nodeK = a.fv_node + (int64_t)kf * a.cap, *offK = a.fv_off + (int64_t)kf * (a.cap + 1),
                   *idxK = a.fv_idx + (int64_t)kf * a.cap;
    const uint32_t *nodeF = a.fv_node + (int64_t)f * a.cap, *offF = a.fv_off + (int64_t)f * (a.cap + 1),
                   *idxF = a.fv_idx + (int64_t)f * a.cap;
    const uint8_t *descK = a.desc + (int64_t)kf * a.cap * 32, *descF = a.desc + (int64_t)f * a.cap * 32;
    const uint8_t *validK = a.valid ? a.valid + (int64_t)kf * a.cap : nullptr;
    const uint8_t *validF = (a.valid && a.use_valid_f) ? a.valid + (int64_t)f * a.cap : nullptr;
    int32_t *match = a.match + (int64_t)p * a.cap;
    for (int an = row; an < nnK; an += nrows) {  // row-uniform
        const uint32_t node = nodeK[an];
        int lo = 0, hi = nnF - 1, b = -1;  // lower_bound walk of :329-333 == binary search on sorted ids
        while (lo <= hi) {
            const int mid = (lo + hi) >> 1;
            const uint32_t v = nodeF[mid];
            if (v == node) { b = mid; break; }
            if (v < node) lo = mid + 1; else hi = mid - 1;
        }
        if (b < 0) continue;
        const uint32_t f0 = offF[b], nFb = offF[b + 1] - f0;
        const uint32_t k0 = offK[an], nKa = offK[an + 1] - k0;
        // chunk 0 of the F list stays in registers
        Desc8 d0;
        uint32_t rf0 = 0;
        bool ok0 = lane16 < (int)nFb;
        if (ok0) {
            rf0 = idxF[f0 + lane16];
            if (validF && !validF[rf0]) ok0 = false;
        }
        d0 = load_desc8(descF + (int64_t)(ok0 ? rf0 : 0) * 32);
        for (uint32_t t = 0; t < nKa; ++t) {
            // the KF features of the node are staged 16 at a time in LDS (index, MapPoint flag, descriptor): the serial
            // loop below then depends on LDS latency only, not on two dependent global loads per feature
            if ((t & 15u) == 0u) {
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // earlier reads of the staging area are done
                uint32_t rk_l = 0xFFFFFFFFu;
                if (t + lane16 < nKa) {
                    rk_l = idxK[k0 + t + lane16];
                    if (validK && !validK[rk_l]) rk_l = 0xFFFFFFFFu;  // !pMP || pMP->isBad() (:256-259)
                }
                s_rk[rowb][lane16] = rk_l;
                const uint4 *pk = (const uint4 *)(descK + (int64_t)(rk_l == 0xFFFFFFFFu ? 0u : rk_l) * 32);
                s_dk[rowb][lane16][0] = pk[0];
                s_dk[rowb][lane16][1] = pk[1];
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            }
            const uint32_t rk = s_rk[rowb][t & 15u];
            if (rk == 0xFFFFFFFFu) continue;
            Desc8 dk;
            {
                const uint4 q0 = s_dk[rowb][t & 15u][0], q1 = s_dk[rowb][t & 15u][1];
                dk.w[0] = q0.x; dk.w[1] = q0.y; dk.w[2] = q0.z; dk.w[3] = q0.w;
                dk.w[4] = q1.x; dk.w[5] = q1.y; dk.w[6] = q1.z; dk.w[7] = q1.w;
            }
            uint32_t b1 = 256, b2 = 256, bpos = 0xFFFFFu;  // running result over the chunks seen so far
            for (uint32_t c0 = 0; c0 < nFb; c0 += 16) {
                uint32_t dist = 0x3FFu;  // "no candidate"
                if (c0 == 0) {
                    if (ok0) {
                        int d = 0;
#pragma unroll
                        for (int i = 0; i < 8; ++i) d += __popc(dk.w[i] ^ d0.w[i]);
                        dist = (uint32_t)d;
                    }
                } else if (c0 + lane16 < nFb) {
                    const uint32_t rf = idxF[f0 + c0 + lane16];
                    const bool free = __hip_atomic_load(&match[rf], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0;
                    if (free && !(validF && !validF[rf])) dist = (uint32_t)hamming8(dk, (const uint32_t *)(descF + (int64_t)rf * 32));
                }
                const uint32_t key = (dist << 20) | (c0 + lane16);        // smaller = closer, earlier position wins ties
                const uint32_t k1 = row_min_u32(key);
                const uint32_t k2 = row_min_u32(key == k1 ? 0xFFFFFFFFu : key);  // best of the OTHER candidates of the chunk
                const uint32_t c1 = k1 >> 20, cs = min(k2 >> 20, 256u), cpos = k1 & 0xFFFFFu;
                if (c1 < 0x3FFu) {   // merge: the running result covers earlier positions (first minimum wins)
                    if (c1 < b1) { b2 = min(b1, cs); b1 = c1; bpos = cpos; }
                    else { b2 = min(b2, c1); }
                }
            }
            const bool pass = a.strict_lt ? ((int)b1 < a.th_low) : ((int)b1 <= a.th_low);
            if (pass && bpos != 0xFFFFFu && (float)b1 < __fmul_rn(a.nnratio, (float)b2)) {
                const uint32_t rf = bpos < 16 ? __shfl(rf0, (threadIdx.x & 48) + (int)bpos, 64) : idxF[f0 + bpos];
                if (lane16 == 0) __hip_atomic_store(&match[rf], (int32_t)rk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");  // later chunk re-reads of this row see the claim
                if (bpos == (uint32_t)lane16) ok0 = false;  // claimed (:273 vpMapPointMatches / :725 vbMatched2)
            }
        }
    }
}

// rotation prune for the batched form: angles come from the keypoint records
__global__ __launch_bounds__(256) void k_rot_prune_bow_batch(BowBatch a)
{
    const int p = blockIdx.x;
    const orbfe_keypoint *kK = a.kps + (int64_t)a.kf[p] * a.cap, *kF = a.kps + (int64_t)a.f[p] * a.cap;
    rot_prune(a.match + (int64_t)p * a.cap, a.cap, a.check_ori, a.nmatches + p, [&](int, int j) { return kK[j].angle; },
              [&](int i, int) { return kF[i].angle; });
}

extern "C" orbfe_status orbfe_bow_transform_batch_device(orbfe_matcher *m, const orbfe_vocabulary *v, const uint8_t *d_desc,
                                                         const int32_t *d_n, int32_t nframes, int32_t cap, int32_t levelsup,
                                                         int32_t *d_f_word, int32_t *d_f_node, double *d_f_weight,
                                                         uint32_t *d_bow_id, double *d_bow_val, uint32_t *d_fv_node,
                                                         uint32_t *d_fv_off, uint32_t *d_fv_idx, int32_t *d_counts,
                                                         void *stream)
{
    if (!m || !v || !d_desc || !d_n || nframes < 1 || cap < 1 || cap > BOW_MAX_FEATURES || !d_f_word || !d_f_node ||
        !d_f_weight || !d_bow_id || !d_bow_val || !d_fv_node || !d_fv_off || !d_fv_idx || !d_counts) {
        orbfe_set_error("bad argument to orbfe_bow_transform_batch_device (cap <= %d)", BOW_MAX_FEATURES);
        return ORBFE_ERR_ARG;
    }
    if (v->device != m->device) { orbfe_set_error("vocabulary and matcher are on different devices"); return ORBFE_ERR_ARG; }
    DeviceGuard g(m->device);
    hipStream_t st = (hipStream_t)stream;
    int P = 2;
    while (P < cap) P <<= 1;
    const size_t lds = (size_t)P * 16;
    hipFuncAttributes fa;
    ORBFE_HIP(hipFuncGetAttributes(&fa, (const void *)k_bow_aggregate));
    const size_t lds_max = (size_t)ORBFE_LDS_MAX - fa.sharedSizeBytes;
    if (lds > lds_max) { orbfe_set_error("orbfe_bow_transform_batch_device: cap %d needs more than the CU's LDS", cap); return ORBFE_ERR_SIZE; }
    if (lds > 64 * 1024)
        ORBFE_HIP(hipFuncSetAttribute((const void *)k_bow_aggregate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
    hipLaunchKernelGGL(k_bow_descend, dim3((cap + 255) / 256, nframes), dim3(256), 0, st, v->child_off.as<const uint32_t>(),
                       v->child_idx.as<const uint32_t>(), v->node_desc.as<const uint8_t>(), v->word_id.as<const uint32_t>(),
                       v->weight.as<const double>(), v->L - levelsup, d_desc, 0, d_f_word, d_f_node, d_f_weight, d_n, cap);
    hipLaunchKernelGGL(k_bow_aggregate, dim3(nframes), dim3(1024), lds, st, 0, P, (const int32_t *)d_f_word,
                       (const int32_t *)d_f_node, (const double *)d_f_weight, d_bow_id, d_bow_val, d_fv_node, d_fv_off,
                       d_fv_idx, d_counts, d_n, cap);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_search_by_bow_batch_device(orbfe_matcher *m, const orbfe_keypoint *d_kps, const uint8_t *d_desc,
                                                         int32_t cap, const uint8_t *d_valid, const uint32_t *d_fv_node,
                                                         const uint32_t *d_fv_off, const uint32_t *d_fv_idx,
                                                         const int32_t *d_counts, const int32_t *d_kf, const int32_t *d_f,
                                                         int32_t npairs, float nnratio, int32_t th_low, int32_t kf_kf,
                                                         int32_t check_ori, int32_t *d_match, int32_t *d_nmatches,
                                                         void *stream)
{
    if (!m || !d_kps || !d_desc || cap < 1 || !d_fv_node || !d_fv_off || !d_fv_idx || !d_counts || !d_kf || !d_f ||
        npairs < 0 || !d_match || !d_nmatches) {
        orbfe_set_error("bad argument to orbfe_search_by_bow_batch_device");
        return ORBFE_ERR_ARG;
    }
    if (npairs == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    hipStream_t st = (hipStream_t)stream;
    BowBatch a;
    a.desc = d_desc; a.kps = d_kps; a.valid = d_valid;
    a.fv_node = d_fv_node; a.fv_off = d_fv_off; a.fv_idx = d_fv_idx; a.counts = d_counts;
    a.kf = d_kf; a.f = d_f;
    a.cap = cap; a.npairs = npairs; a.th_low = th_low; a.strict_lt = kf_kf ? 1 : 0; a.use_valid_f = kf_kf ? 1 : 0;
    a.check_ori = check_ori; a.nnratio = nnratio;
    a.match = d_match; a.nmatches = d_nmatches;
    ORBFE_HIP(hipMemsetAsync(d_match, 0xFF, sizeof(int32_t) * (size_t)npairs * cap, st));
    hipLaunchKernelGGL(k_search_by_bow_rows, dim3(8, npairs), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_rot_prune_bow_batch, dim3(npairs), dim3(256), 0, st, a);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}

// ---------------------------------------------------------------------------------------------------
// SURVEY 8(f).4  MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:284-345), batched over map points.
// One wave per map point: its observed descriptors are staged in LDS, lane i owns row i of the distance matrix and
// finds that row's median -- element (int)(0.5 * (N - 1)) of the sorted row, self distance 0 included (:332-334) --
// by bisection on the value range [0, 256] with the row recomputed from LDS (no N x N matrix, any N); the point's
// descriptor is the row with the least median, first on ties (:335-339).
// ---------------------------------------------------------------------------------------------------
#define DD_MAX_OBS 1024

__global__ __launch_bounds__(64) void k_distinctive(const uint8_t *__restrict__ pool, const uint32_t *__restrict__ off,
                                                    const uint32_t *__restrict__ idx, int32_t *__restrict__ best_idx,
                                                    int32_t *__restrict__ median, int max_obs)
{
    extern __shared__ uint4 s_obs[];  // [max_obs][2]
    const int p = blockIdx.x, lane = threadIdx.x;
    const uint32_t o0 = off[p];
    const int n = (int)(off[p + 1] - o0);
    if (n <= 0 || n > max_obs) {  // no observation: -1; more than the LDS was sized for (device entry point only): -2
        if (lane == 0) { best_idx[p] = n <= 0 ? -1 : -2; median[p] = n <= 0 ? -1 : -2; }
        return;
    }
    for (int t = lane; t < 2 * n; t += 64) s_obs[t] = ((const uint4 *)pool)[(size_t)idx[o0 + (t >> 1)] * 2 + (t & 1)];
    __syncthreads();
    const int k = (int)(0.5 * (n - 1));
    uint32_t bestkey = 0xFFFFFFFFu;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane, ic = min(i, n - 1);
        const uint4 a0 = s_obs[2 * ic], a1 = s_obs[2 * ic + 1];
        int lo = 0, hi = 256;
        for (int it = 0; it < 9; ++it) {  // 257 values: 9 halvings; lanes whose interval closed early idle harmlessly
            const int mid = (lo + hi) >> 1;
            int cnt = 0;
            for (int j = 0; j < n; ++j) {
                const uint4 b0 = s_obs[2 * j], b1 = s_obs[2 * j + 1];  // same address in every lane: LDS broadcast
                const int d = __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
                              __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
                cnt += d <= mid ? 1 : 0;
            }
            if (lo < hi) {
                if (cnt >= k + 1) hi = mid;
                else lo = mid + 1;
            }
        }
        if (i < n) bestkey = min(bestkey, ((uint32_t)lo << 16) | (uint32_t)i);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bestkey = min(bestkey, (uint32_t)__shfl_xor((int)bestkey, o, 64));
    if (lane == 0) {
        best_idx[p] = (int32_t)(bestkey & 0xFFFFu);
        median[p] = (int32_t)(bestkey >> 16);
    }
}

extern "C" orbfe_status orbfe_distinctive_descriptors(orbfe_matcher *m, const uint8_t *pool, int32_t npool,
                                                      const uint32_t *off, const uint32_t *idx, int32_t npoints,
                                                      int32_t *best_idx, int32_t *median)
{
    if (!m || npool < 0 || npoints < 0 || (npoints > 0 && (!off || !best_idx || !median))) {
        orbfe_set_error("bad argument to orbfe_distinctive_descriptors");
        return ORBFE_ERR_ARG;
    }
    if (npoints == 0) return ORBFE_OK;
    uint32_t maxn = 0;
    for (int i = 0; i < npoints; ++i) {
        if (off[i + 1] < off[i]) { orbfe_set_error("CSR offsets must not decrease"); return ORBFE_ERR_ARG; }
        maxn = std::max(maxn, off[i + 1] - off[i]);
    }
    if (maxn > DD_MAX_OBS) {
        orbfe_set_error("a map point with %u observations exceeds the supported %d", maxn, DD_MAX_OBS);
        return ORBFE_ERR_ARG;
    }
    const size_t nc = off[npoints];
    if (nc > 0 && (!idx || !pool)) { orbfe_set_error("null pool / idx"); return ORBFE_ERR_ARG; }
    for (size_t k = 0; k < nc; ++k)
        if (idx[k] >= (uint32_t)npool) { orbfe_set_error("observation index out of range"); return ORBFE_ERR_ARG; }
    DeviceGuard g(m->device);
    hipStream_t st = m->stream;
    ORBFE_HIP(scratch_acquire(m, st));  // a device-buffer call on another stream may still be using the scratch blocks
    ORBFE_HIP(m->b[0].ensure((size_t)std::max(npool, 1) * 32));
    ORBFE_HIP(m->b[2].ensure((size_t)(npoints + 1) * 4));
    ORBFE_HIP(m->b[3].ensure(std::max(nc, (size_t)1) * 4));
    ORBFE_HIP(m->b[4].ensure((size_t)npoints * 4));
    ORBFE_HIP(m->b[5].ensure((size_t)npoints * 4));
    if (npool > 0) ORBFE_HIP(hipMemcpyAsync(m->b[0].p, pool, (size_t)npool * 32, hipMemcpyHostToDevice, st));
    ORBFE_HIP(hipMemcpyAsync(m->b[2].p, off, (size_t)(npoints + 1) * 4, hipMemcpyHostToDevice, st));
    if (nc > 0) ORBFE_HIP(hipMemcpyAsync(m->b[3].p, idx, nc * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_distinctive, dim3(npoints), dim3(64), (size_t)std::max(maxn, 1u) * 32, st,
                       m->b[0].as<const uint8_t>(), m->b[2].as<const uint32_t>(), m->b[3].as<const uint32_t>(),
                       m->b[4].as<int32_t>(), m->b[5].as<int32_t>(), (int)std::max(maxn, 1u));
    ORBFE_HIP(hipGetLastError());
    ORBFE_HIP(hipMemcpyAsync(best_idx, m->b[4].p, (size_t)npoints * 4, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipMemcpyAsync(median, m->b[5].p, (size_t)npoints * 4, hipMemcpyDeviceToHost, st));
    ORBFE_HIP(hipStreamSynchronize(st));
    return ORBFE_OK;
}

extern "C" orbfe_status orbfe_distinctive_descriptors_device(orbfe_matcher *m, const uint8_t *d_pool, const uint32_t *d_off,
                                                             const uint32_t *d_idx, int32_t npoints, int32_t max_obs,
                                                             int32_t *d_best_idx, int32_t *d_median, void *stream)
{
    if (!m || npoints < 0 || max_obs < 1 || max_obs > DD_MAX_OBS || (npoints > 0 && (!d_pool || !d_off || !d_idx || !d_best_idx || !d_median))) {
        orbfe_set_error("bad argument to orbfe_distinctive_descriptors_device (max_obs 1..%d)", DD_MAX_OBS);
        return ORBFE_ERR_ARG;
    }
    if (npoints == 0) return ORBFE_OK;
    DeviceGuard g(m->device);
    hipLaunchKernelGGL(k_distinctive, dim3(npoints), dim3(64), (size_t)max_obs * 32, (hipStream_t)stream, d_pool, d_off, d_idx, d_best_idx,
                       d_median, max_obs);
    ORBFE_HIP(hipGetLastError());
    return ORBFE_OK;
}
