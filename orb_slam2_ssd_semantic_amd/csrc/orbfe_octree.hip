// orbfe_octree.hip -- K3, DistributeOctTree on the device (k_octree).
#include "orbfe_kernels_dev.h"
#include "orbfe_host.h"

// ---------------------------------------------------------------------------------------------------
// K3  DistributeOctTree on the device.  One workgroup per (frame, level).
//
// The reference keeps a std::list of nodes: a pass visits nodes in some processing order, replaces each
// visited node by its non-empty children (push_front in the order n1,n2,n3,n4) and may stop early once
// the list holds >= N nodes.  Both of its loops are instances of one generic pass:
//     breadth-first loop (:608-667)  processing order = list order,           never stops early
//     largest-first loop (:678-739)  processing order = (size desc, creation desc), stops at >= N
// and the list after a pass that processed ranks 0..R-1 is
//     [children(P[R-1]) n4..n1] ... [children(P[0]) n4..n1]  ++  [unprocessed nodes in old order].
// Positions therefore follow from prefix sums over the processing order and the final "first strongest key" from an
// LDS atomicMax on (response | ~candidate_order | key index).  Keys never move.
// Equal-size ties in the largest-first order are broken by creation order (the reference compares heap
// addresses there, :686 -- see DESIGN.md "quadtree contract").
//
// What a pass needs from the keys is only the number of keys in each child quadrant.  The child boxes are a pure
// function of the root box (DivideNode halves with ceil, :480-481), so every key's quadrant path is known up front:
// the prologue computes a 5-level path code per key and a histogram over the 4^5 leaves of every root; quadrant
// counts of any node down to depth 4 are sums of that histogram.  The first 5 passes -- normally all of them --
// therefore run as node-level bookkeeping only, by ONE wave, without touching the keys and without barriers.
// Only trees that must go deeper fall back to streaming key passes (keys then carry their node index).
// Keys arrive in arbitrary order from k_fast_map; each carries `ord`, its rank in the reference's candidate order.
// ---------------------------------------------------------------------------------------------------
#define QT_MAX 512
// One launch covers a run of consecutive levels whose node lists, root counts and path tables share one LDS carve-up:
// the upper pyramid levels ask for a fraction of level 0's features, so their workgroups are given a smaller carve-up
// and fewer threads and more of them fit a CU (the node bookkeeping is one wave's serial work per workgroup).
struct OctGroup {
    int32_t level0;        // first level of the group; gridDim.x = number of levels in it
    int32_t M;             // node capacity (multiple of 64)
    int32_t nini;          // most roots of a level in the group
    int32_t tw, th;        // largest level size in the group (path tables)
    int32_t ncells;        // most FAST cells of a level in the group
};
#define KNODE_MASK 0x3FFFu
#ifndef KUNROLL
#define KUNROLL 8
#endif
#define FFD 5               // histogram depth
#define FF_PER_ROOT 1364    // 4 + 16 + 64 + 256 + 1024
__host__ __device__ inline int ff_off(int d) { return ((1 << (2 * d)) - 4) / 3; }  // first entry of depth d (1..5)

struct QtShared {
    // two generations of the node list (current / next), addressed arithmetically -- an array of pointers indexed by
    // a run-time generation would live in scratch memory
    int M;
    int32_t *cnt0;       // [2][M]
    uint32_t *path0;     // [2][M] prefix | depth << 12 | root << 16
    __device__ __forceinline__ int32_t *cnt(int g) const { return cnt0 + g * M; }
    __device__ __forceinline__ uint32_t *path(int g) const { return path0 + g * M; }
    // [M*4] quadrant counts of the current pass; the node phase turns the entry of (node, quadrant) into the position of
    // that child in the next list (-1 if empty): the same words, read as `cc` before and as `childpos` after
    int32_t *cc;
    int32_t *P;          // processing order -> node index
    int32_t *rankOf0;    // [2][M] node index -> processing rank or -1 (per list generation)
    __device__ __forceinline__ int32_t *rankOf(int g) const { return rankOf0 + g * M; }
    int32_t *acc;        // inclusive sums over ranks
    int32_t *newIdx;     // next-list position of an unprocessed node, -1 for a processed one
    unsigned long long *skey;
    int32_t *hist;       // [nroots * FF_PER_ROOT] quadrant-path histogram, later the path -> node table
    uint16_t *xtab;      // [w] window column -> root << 10 | x half of the 5-level path code (bits 8,6,4,2,0)
    uint16_t *ytab;      // [h] window row    -> y half of the path code (bits 9,7,5,3,1)
    uint32_t *cflag;     // [ncells / 32] bit = the FAST cell has a survivor above iniTh
    int32_t *misc;       // [64]: 0..15 state, 16..23 root slots, 32..49 scan scratch
    // node boxes exist only for trees that go deeper than the histogram (clustered candidates): two generations of
    // (ulx, uly, urx, bry) in GLOBAL scratch of this (frame, level) -- [2][4][M] int16
    int16_t *gbox;
    __device__ __forceinline__ int16_t *box(int g, int j) const { return gbox + (g * 4 + j) * M; }
};

__host__ __device__ inline int qt_pow2(int v)
{
    int p = 2;
    while (p < v) p <<= 1;
    return p;
}

// The node arrays (56 B per node + the sort buffer) normally live in LDS next to the histogram and the tables; a level that
// asks for more nodes than the CU's LDS holds (nfeatures beyond ~2400 per level) keeps them in a global scratch slice of its
// (frame, level) instead -- same code, the accesses become global loads / stores (template parameter of k_octree).
__device__ __forceinline__ void qt_carve(char *lds, char *nodes, int M, int nroots, int w, int h, int ncells, QtShared &q)
{
    char *p = nodes;
    q.skey = (unsigned long long *)p; p += (size_t)qt_pow2(M) * 8;  // the largest-first sort is bitonic: power of two
    q.cc = (int32_t *)p; p += (size_t)M * 16;
    q.M = M;
    q.cnt0 = (int32_t *)p; p += (size_t)M * 8;
    q.path0 = (uint32_t *)p; p += (size_t)M * 8;
    q.P = (int32_t *)p; p += (size_t)M * 4;
    q.rankOf0 = (int32_t *)p; p += (size_t)M * 8;
    q.acc = (int32_t *)p; p += (size_t)M * 4;
    q.newIdx = (int32_t *)p; p += (size_t)M * 4;
    p = nodes == lds ? p : lds;
    q.hist = (int32_t *)p; p += (size_t)nroots * FF_PER_ROOT * 4;
    q.misc = (int32_t *)p; p += 64 * 4;
    q.xtab = (uint16_t *)p; p += (size_t)((w + 1) & ~1) * 2;
    q.ytab = (uint16_t *)p; p += (size_t)((h + 1) & ~1) * 2;
    q.cflag = (uint32_t *)p;
}

size_t orbk_octree_node_bytes(int M) { return orb_align256((size_t)qt_pow2(M) * 8 + (size_t)M * (16 + 8 + 8 + 20)); }
static size_t octree_table_bytes(int nroots, int w, int h, int ncells)
{
    return (size_t)nroots * FF_PER_ROOT * 4 + 64 * 4 + (size_t)(((w + 1) & ~1) + ((h + 1) & ~1)) * 2 + (size_t)((ncells + 31) / 32) * 4;
}
size_t orbk_octree_lds_bytes(int M, int nroots, int w, int h, int ncells)
{
    return (size_t)qt_pow2(M) * 8 + (size_t)M * (16 + 8 + 8 + 20) + octree_table_bytes(nroots, w, h, ncells);
}

// bytes of global scratch one (frame, level) workgroup may need for the node boxes of a deep tree
size_t orbk_octree_box_bytes(int M) { return (size_t)M * 2 * 4 * sizeof(int16_t); }

__device__ __forceinline__ int wave_min_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// inclusive scan of arr[0..n) in LDS, in place, by all threads of the workgroup; returns the total.  Ends with a barrier.
__device__ __forceinline__ int bscan_inclusive(int32_t *arr, int n, int32_t *sw)
{
    const int tid = threadIdx.x, QT = blockDim.x, wid = tid >> 6, lane = tid & 63, nw = QT >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += QT) {
        const int i = base + tid;
        const int v = i < n ? arr[i] : 0;
        const int incl = wave_incl_scan(v);
        if (lane == 63) sw[wid] = incl;
        __syncthreads();
        int pre = 0, tot = 0;
        for (int w = 0; w < nw; ++w) {
            const int t = sw[w];
            pre += w < wid ? t : 0;
            tot += t;
        }
        if (i < n) arr[i] = carry + pre + incl;
        carry += tot;
        __syncthreads();
    }
    return carry;
}

// One generic pass at node level, executed by ALL threads of the workgroup (barriers between its steps).
// In:  q.cc[i*4+qd] for every node i in P (quadrant sizes), list `cur` of size S, processing order P[0..m), rankOf.
// Out: list `cur^1` (sizes, paths; boxes when DEEP), the old->new map (newIdx / cc-as-childpos), next P / rankOf, S, m,
//      modeB, finish -- all workgroup-uniform.
// largest-first processing order (:686-687): q.skey[0..Mp) holds (size << 32 | (creation seq + 1) << 16 | list position) for
// the nToExpand multi-key children (zero beyond); sorts descending and writes P / rankOf of list generation nx
__device__ __forceinline__ void qt_sort_assign(const QtShared &q, int Mp, int nToExpand, int S2, int nx)
{
    const int tid = threadIdx.x, QT = blockDim.x;
    for (int kk = 2; kk <= Mp; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < Mp; i += QT) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = q.skey[i], c2 = q.skey[ixj];
                    const bool desc = (i & kk) == 0;  // overall descending
                    if (desc ? (a < c2) : (a > c2)) { q.skey[i] = c2; q.skey[ixj] = a; }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < S2; i += QT) q.rankOf(nx)[i] = -1;
    __syncthreads();
    for (int r = tid; r < nToExpand; r += QT) {
        const int pos = (int)(q.skey[r] & 0xFFFFull);
        q.P[r] = pos;
        q.rankOf(nx)[pos] = r;
    }
}

// Two inclusive scans with shared barriers: a[0..na) and b[0..nb) in LDS, in place, by all threads.  Ends with a barrier.
__device__ __forceinline__ void bscan2_inclusive(int32_t *a, int na, int32_t *b, int nb, int32_t *sw, int &ta, int &tb)
{
    const int tid = threadIdx.x, QT = blockDim.x, wid = tid >> 6, lane = tid & 63, nw = QT >> 6;
    int ca = 0, cb = 0;
    for (int base = 0; base < max(na, nb); base += QT) {
        const int i = base + tid;
        const int va = i < na ? a[i] : 0, vb = i < nb ? b[i] : 0;
        const int ia = wave_incl_scan(va), ib = wave_incl_scan(vb);
        if (lane == 63) { sw[wid] = ia; sw[8 + wid] = ib; }
        __syncthreads();
        int pa = 0, pb = 0, sa = 0, sb = 0;
        for (int w = 0; w < nw; ++w) {
            const int x = sw[w], y = sw[8 + w];
            pa += w < wid ? x : 0;
            pb += w < wid ? y : 0;
            sa += x;
            sb += y;
        }
        if (i < na) a[i] = ca + pa + ia;
        if (i < nb) b[i] = cb + pb + ib;
        ca += sa;
        cb += sb;
        __syncthreads();
    }
    ta = ca;
    tb = cb;
}

// A breadth-first pass (:608-667) of a tree whose node sizes come from the leaf histogram: every multi-key node of the list
// is split, in list order.  Same result as qt_node_phase<false> with modeB == 0, in 4 barriers instead of 15: children
// and multi-key-children counts per rank are scanned together (packed), the unprocessed-node flags in the same barrier pair,
// and the next processing order (list order of the new multi-key nodes, or the sort keys when the largest-first mode
// begins) is written together with the next list -- a multi-key child of rank r sits at multi-rank
// totalMulti - inclMulti[r] + (its index among r's multi-key children in n4..n1 order), creation sequence
// inclMulti[r] - nMulti[r] + (index in n1..n4 order).
__device__ __forceinline__ void qt_pass_bfs_hist(const QtShared &q, int N, int &S, int &m, int &cur, int &modeB, bool &finish)
{
    const int tid = threadIdx.x, QT = blockDim.x;
    const int nx = cur ^ 1;
    int32_t *sw = q.misc + 32;
    int32_t *pk = q.acc, *un = q.newIdx;
    auto quad = [&](int i) {
        const uint32_t pth = q.path(cur)[i];
        const int d = (int)((pth >> 12) & 0xFu), root = (int)(pth >> 16);
        return &q.hist[root * FF_PER_ROOT + ff_off(d + 1) + (int)((pth & 0xFFFu) << 2)];
    };
    for (int r = tid; r < m; r += QT) {
        const int32_t *c = quad(q.P[r]);
        pk[r] = ((c[0] > 0) + (c[1] > 0) + (c[2] > 0) + (c[3] > 0)) | (((c[0] > 1) + (c[1] > 1) + (c[2] > 1) + (c[3] > 1)) << 16);
    }
    for (int i = tid; i < S; i += QT) un[i] = q.rankOf(cur)[i] < 0 ? 1 : 0;
    __syncthreads();
    int tpk, nUnproc;
    bscan2_inclusive(pk, m, un, S, sw, tpk, nUnproc);
    const int totalChildren = tpk & 0xFFFF, nToExpand = tpk >> 16;
    const int S2 = totalChildren + nUnproc;
    finish = (S2 >= N) || (S2 == S);  // :671
    const int modeB2 = (!finish && (S2 + 3 * nToExpand > N)) ? 1 : 0;  // :675
    int Mp = 2;
    if (modeB2) {
        while (Mp < nToExpand) Mp <<= 1;
        for (int i = tid; i < Mp; i += QT) q.skey[i] = 0ull;
        __syncthreads();
    }
    for (int i = tid; i < S; i += QT) {
        const int r = q.rankOf(cur)[i];
        const uint32_t pth = q.path(cur)[i];
        if (r >= 0) {
            const int inc = pk[r];
            const int32_t *c = quad(i);
            const int c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
            const int cn[4] = {c0, c1, c2, c3};
            int pos = totalChildren - (inc & 0xFFFF);
            int mr = nToExpand - (inc >> 16);                                                 // multi-rank of the first multi-key child in list order
            int seq = (inc >> 16) - ((c0 > 1) + (c1 > 1) + (c2 > 1) + (c3 > 1));              // creation sequence of n1's slot
            int seqq[4];
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) { seqq[qd] = seq; seq += cn[qd] > 1 ? 1 : 0; }
            const uint32_t cpath = (pth & 0xFFFF0000u) | ((((pth >> 12) & 0xFu) + 1u) << 12) | ((pth & 0xFFFu) << 2);
#pragma unroll
            for (int qd = 3; qd >= 0; --qd) {  // list front holds n4, then n3, n2, n1 (:623-662)
                if (cn[qd] > 0) {
                    q.cnt(nx)[pos] = cn[qd];
                    q.path(nx)[pos] = cpath | (uint32_t)qd;
                    if (cn[qd] > 1) {
                        if (modeB2) {
                            q.skey[seqq[qd]] = ((unsigned long long)(uint32_t)cn[qd] << 32) |
                                               ((unsigned long long)(uint32_t)(seqq[qd] + 1) << 16) | (unsigned long long)pos;
                        } else {
                            q.P[mr] = pos;
                            q.rankOf(nx)[pos] = mr;
                        }
                        ++mr;
                    } else if (!modeB2) {
                        q.rankOf(nx)[pos] = -1;
                    }
                    ++pos;
                }
            }
        } else {
            const int pos = totalChildren + un[i] - 1;
            q.cnt(nx)[pos] = q.cnt(cur)[i];
            q.path(nx)[pos] = pth;
            if (!modeB2) q.rankOf(nx)[pos] = -1;
        }
    }
    __syncthreads();
    if (!finish && modeB2) qt_sort_assign(q, Mp, nToExpand, S2, nx);
    __syncthreads();
    S = S2;
    m = finish ? 0 : nToExpand;
    cur = nx;
    modeB = modeB2;
}

template <bool DEEP>
__device__ __forceinline__ void qt_node_phase(const QtShared &q, int N, int &S, int &m, int &cur, int &modeB, bool &finish)
{
    const int tid = threadIdx.x, QT = blockDim.x, lane = tid & 63;
    const int nx = cur ^ 1;
    int32_t *sw = q.misc + 32;
    int32_t *childpos = q.cc;
    // non-empty children per processing rank, inclusive sums, stop rank R
    for (int r = tid; r < m; r += QT) {
        const int i = q.P[r];
        q.acc[r] = (q.cc[i * 4] > 0) + (q.cc[i * 4 + 1] > 0) + (q.cc[i * 4 + 2] > 0) + (q.cc[i * 4 + 3] > 0);
    }
    if (tid == 0) q.misc[6] = m;
    __syncthreads();
    bscan_inclusive(q.acc, m, sw);
    int R = m;
    if (modeB) {  // first rank whose split brings the list to >= N nodes (:732)
        int rmin = m;
        for (int r = tid; r < m; r += QT)
            if (S + q.acc[r] - (r + 1) >= N) rmin = min(rmin, r + 1);
        rmin = wave_min_i(rmin);
        if (lane == 0 && rmin < m) atomicMin(&q.misc[6], rmin);
        __syncthreads();
        R = q.misc[6];
    }
    const int totalChildren = R > 0 ? q.acc[R - 1] : 0;
    // unprocessed nodes keep their relative order behind the new children
    for (int i = tid; i < S; i += QT) {
        const int r = q.rankOf(cur)[i];
        q.newIdx[i] = (r >= 0 && r < R) ? 0 : 1;
    }
    __syncthreads();
    const int nUnproc = bscan_inclusive(q.newIdx, S, sw);
    const int S2 = totalChildren + nUnproc;
    // write the next list; leave the old->new map (newIdx / childpos) for whoever follows the keys
    for (int i = tid; i < S; i += QT) {
        const int r = q.rankOf(cur)[i];
        const uint32_t pth = q.path(cur)[i];
        if (r >= 0 && r < R) {
            int pos = totalChildren - q.acc[r];
            int ulx = 0, uly = 0, urx = 0, bry = 0, midx = 0, midy = 0;
            if (DEEP) {
                ulx = q.box(cur, 0)[i]; uly = q.box(cur, 1)[i];
                urx = q.box(cur, 2)[i]; bry = q.box(cur, 3)[i];
                midx = ulx + ((urx - ulx + 1) >> 1); midy = uly + ((bry - uly + 1) >> 1);  // ceil(w/2) (:480-481)
            }
            const uint32_t cpath = (pth & 0xFFFF0000u) | ((((pth >> 12) & 0xFu) + 1u) << 12) | ((pth & 0xFFFu) << 2);
            for (int qd = 3; qd >= 0; --qd) {  // list front holds n4, then n3, n2, n1 (:623-662)
                const int cn = q.cc[i * 4 + qd];
                if (cn > 0) {
                    if (DEEP) {
                        q.box(nx, 0)[pos] = (int16_t)((qd & 1) ? midx : ulx);
                        q.box(nx, 1)[pos] = (int16_t)((qd & 2) ? midy : uly);
                        q.box(nx, 2)[pos] = (int16_t)((qd & 1) ? urx : midx);
                        q.box(nx, 3)[pos] = (int16_t)((qd & 2) ? bry : midy);
                    }
                    q.cnt(nx)[pos] = cn;
                    q.path(nx)[pos] = cpath | (uint32_t)qd;
                    childpos[i * 4 + qd] = pos;
                    ++pos;
                } else {
                    childpos[i * 4 + qd] = -1;
                }
            }
            q.newIdx[i] = -1;
        } else {
            const int pos = totalChildren + q.newIdx[i] - 1;
            if (DEEP) {
                q.box(nx, 0)[pos] = q.box(cur, 0)[i];
                q.box(nx, 1)[pos] = q.box(cur, 1)[i];
                q.box(nx, 2)[pos] = q.box(cur, 2)[i];
                q.box(nx, 3)[pos] = q.box(cur, 3)[i];
            }
            q.cnt(nx)[pos] = q.cnt(cur)[i];
            q.path(nx)[pos] = pth;
            q.newIdx[i] = pos;
        }
    }
    __syncthreads();
    // multi-key children in creation order (rank asc, n1..n4): counts per rank -> sequence numbers
    for (int r = tid; r < R; r += QT) {
        const int i = q.P[r];
        int mc = 0;
        for (int qd = 0; qd < 4; ++qd) {
            const int pos = childpos[i * 4 + qd];
            if (pos >= 0 && q.cnt(nx)[pos] > 1) ++mc;
        }
        q.acc[r] = mc;
    }
    __syncthreads();
    const int nToExpand = bscan_inclusive(q.acc, R, sw);
    // termination / next mode (:671-675, :736)
    finish = (S2 >= N) || (S2 == S);
    int modeB2 = modeB;
    if (!modeB && !finish && (S2 + 3 * nToExpand > N)) modeB2 = 1;
    int m2 = 0;
    if (!finish) {
        if (!modeB2) {
            // list order of the multi-key nodes of the new list; P/rankOf of the OLD list are dead now
            int32_t *flag = (int32_t *)q.skey;
            for (int i = tid; i < S2; i += QT) flag[i] = q.cnt(nx)[i] > 1 ? 1 : 0;
            __syncthreads();
            m2 = bscan_inclusive(flag, S2, sw);
            for (int i = tid; i < S2; i += QT) {
                const bool multi = q.cnt(nx)[i] > 1;
                const int r = flag[i] - 1;
                q.rankOf(nx)[i] = multi ? r : -1;
                if (multi) q.P[r] = i;
            }
        } else {
            // sort the new multi-key children by (size desc, creation seq desc) (:686-687)
            int Mp = 2;
            while (Mp < nToExpand) Mp <<= 1;
            for (int i = tid; i < Mp; i += QT) q.skey[i] = 0ull;
            __syncthreads();
            for (int r = tid; r < R; r += QT) {
                const int i = q.P[r];
                int mc = 0;
                for (int qd = 0; qd < 4; ++qd) {
                    const int pos = childpos[i * 4 + qd];
                    if (pos >= 0 && q.cnt(nx)[pos] > 1) ++mc;
                }
                int seq = q.acc[r] - mc;  // acc is inclusive
                for (int qd = 0; qd < 4; ++qd) {
                    const int pos = childpos[i * 4 + qd];
                    if (pos >= 0 && q.cnt(nx)[pos] > 1) {
                        q.skey[seq] = ((unsigned long long)(uint32_t)q.cnt(nx)[pos] << 32) |
                                      ((unsigned long long)(uint32_t)(seq + 1) << 16) | (unsigned long long)pos;
                        ++seq;
                    }
                }
            }
            __syncthreads();
            qt_sort_assign(q, Mp, nToExpand, S2, nx);
            m2 = nToExpand;
        }
    }
    __syncthreads();
    S = S2;
    m = m2;
    cur = nx;
    modeB = modeB2;
}

// -DQT_PROFILE: per-phase clock stamps of k_octree summed into OrbMisc::qt_phase (orbfe_extractor.h: 64 bytes behind the overflow
// word, eight 64-bit sums per level; developer builds only; read with orbfe_internal_read_misc, tools/octree_phases.py)
#ifdef QT_PROFILE
#define QT_STAMP(p)                                                                                              \
    do {                                                                                                         \
        if (tid == 0) {                                                                                          \
            const unsigned long long t_now = wall_clock64();                                                     \
            atomicAdd((unsigned long long *)ovf + 8 + (p) + 8 * min(level, 14), t_now - t_prev);               \
            t_prev = t_now;                                                                                      \
        }                                                                                                        \
    } while (0)
#else
#define QT_STAMP(p)
#endif
#ifndef QT_MIN_WAVES
#define QT_MIN_WAVES 6   // waves per SIMD the register allocation must allow (A/B on the GPU box: tools/ab_build.sh)
#endif
template <bool GNODES>
__global__ __launch_bounds__(QT_MAX, QT_MIN_WAVES) void k_octree(const OrbPlan *__restrict__ plan,
                                               const uint2 *__restrict__ skeys,     // [B][keys_per_frame] {key, ord} from k_fast_map
                                               const int32_t *__restrict__ scount,  // [B][nlevels] * NK_STRIDE
                                               const uint32_t *__restrict__ cflags, // [B][nlevels][cf_words] from k_fast_map
                                               int32_t cf_words,
                                               uint16_t *__restrict__ knode,        // [B][keys_per_frame] scratch (deep trees only)
                                               int16_t *__restrict__ qtbox,         // [B][nlevels][box_stride] scratch (deep trees only)
                                               int32_t box_stride,
                                               char *__restrict__ qtnodes,          // [B][nlevels][node_stride] node arrays (GNODES only)
                                               int64_t node_stride,
                                               int32_t *__restrict__ nkeys,         // [B][nlevels] out (taps)
                                               uint32_t *__restrict__ sel,          // [B][sel_per_frame] out
                                               int32_t *__restrict__ nsel,          // [B][nlevels] out
                                               int32_t *__restrict__ ovf,           // sticky overflow word
                                               OctGroup g)                          // the levels this launch covers
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // Workgroups go round-robin to the 8 XCDs in launch order; with level = blockIdx.x every XCD would own ONE pyramid
    // level of all frames, and level 0 carries ~10x the keys of level 7.  Rotating the level by the frame index gives
    // every XCD the same mix of levels.
    const int b = blockIdx.y, level = g.level0 + (int)((blockIdx.x + blockIdx.y) % gridDim.x), tid = threadIdx.x;
    const int lane = tid & 63;
    const int QT = blockDim.x;  // 128 .. 512 (per level group)
    const OrbLevel &L = plan->lv[level];
    const int N = L.nfeat;
    QtShared q;
    qt_carve(smem, GNODES ? qtnodes + ((int64_t)b * plan->nlevels + level) * node_stride : smem, g.M, g.nini, g.tw, g.th, g.ncells, q);
    q.gbox = qtbox + ((int64_t)b * plan->nlevels + level) * box_stride;
    int32_t *misc = q.misc;
    const uint2 *SK = skeys + (int64_t)b * plan->keys_per_frame + L.key_off;
    uint16_t *KN = knode + (int64_t)b * plan->keys_per_frame + L.key_off;
    const int nini = L.nini;
    const int ybot = L.h - 2 * ORBFE_MINB;  // maxBorderY - minBorderY
#ifdef QT_PROFILE
    unsigned long long t_prev = wall_clock64();
#endif

    // ---- prologue 1: the reference's per-cell threshold fallback (:818-825): a cell contributes {A > iniTh} if that is
    // non-empty, else all its NMS survivors ({A > minTh}).  Which cells have an iniTh survivor was recorded by k_fast_map as
    // it emitted them (one bit per cell): no pass over the keys is spent on it here.
    const int ns_all = scount[(b * plan->nlevels + level) * ORBFE_NK_STRIDE];
    const int ns = min(ns_all, L.key_cap);
    if (tid == 0 && ns_all > L.key_cap) atomicOr(ovf, 1);  // k_fast_map dropped survivors: results would be truncated
    uint32_t *cflag = q.cflag;  // bitmap over this level's cells; stays valid to the end of the kernel
    const int nwords = (L.ncells + 31) >> 5;
    {
        const uint32_t *gflag = cflags + (int64_t)(b * plan->nlevels + level) * cf_words;
        for (int i = tid; i < nwords; i += QT) cflag[i] = gflag[i];
    }
    for (int i = tid; i < nini * FF_PER_ROOT; i += QT) q.hist[i] = 0;
    if (tid == 0) misc[5] = 0;
    // DivideNode (:478-522) halves x and y independently (mid = UL + ceil(extent / 2)), so a key's 5-level quadrant
    // path is the bit-interleave of a 5-level x path (a function of the key's column and root) and a 5-level y path
    // (a function of its row): two small tables replace five DivideNode steps per key.
    const int winw = L.w - 2 * ORBFE_MINB;
    for (int i = tid; i < winw + ybot; i += QT) {
        const bool isx = i < winw;
        const int v = isx ? i : i - winw;
        int lo = 0, hi = ybot, r = 0;
        if (isx) {  // roots (:545-571): key -> root by (int)(x / hX)
            r = (int)__fdiv_rn((float)v, L.hx);
            r = min(max(r, 0), nini - 1);
            lo = L.root_x[r];
            hi = L.root_x[r + 1];
        }
        uint32_t code = 0;
#pragma unroll
        for (int d = 0; d < FFD; ++d) {
            const int mid = lo + ((hi - lo + 1) >> 1);
            const int hb = v < mid ? 0 : 1;
            code = (code << 2) | (uint32_t)hb;
            lo = hb ? mid : lo;
            hi = hb ? hi : mid;
        }
        if (isx) q.xtab[v] = (uint16_t)(((uint32_t)r << 10) | code);
        else q.ytab[v] = (uint16_t)(code << 1);
    }
    __syncthreads();
    QT_STAMP(0);
    const int ini = plan->ini_th;
    QT_STAMP(1);
    // ---- prologue 2: leaf histogram of the kept keys (a key is kept if it is above iniTh or its cell has no such key).
    // Keys are never moved or copied: whoever needs a key later re-derives "kept" and its path code from the key.
    auto key_kept = [&](const uint2 &e) {
        const uint32_t cell = e.y >> 12;
        return (int)orb_key_r(e.x) >= ini || !((cflag[cell >> 5] >> (cell & 31)) & 1u);
    };
    auto key_code = [&](const uint2 &e) {  // root << 10 | 5-level path code
        return (uint32_t)q.xtab[orb_key_x(e.x)] | (uint32_t)q.ytab[orb_key_y(e.x)];
    };
    int nkept = 0;
    for (int k0 = tid; k0 < ns; k0 += QT * KUNROLL) {
        uint2 e[KUNROLL];
#pragma unroll
        for (int u = 0; u < KUNROLL; ++u) e[u] = SK[min(k0 + u * QT, ns - 1)];
#pragma unroll
        for (int u = 0; u < KUNROLL; ++u)
            if (k0 + u * QT < ns && key_kept(e[u])) {
                const uint32_t rc = key_code(e[u]);
                atomicAdd(&q.hist[(int)(rc >> 10) * FF_PER_ROOT + ff_off(FFD) + (int)(rc & 0x3FFu)], 1);
                ++nkept;
            }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nkept += __shfl_xor(nkept, o, 64);
    if (lane == 0 && nkept) atomicAdd(&misc[5], nkept);
    __syncthreads();
    const int n = misc[5];
    if (tid == 0) nkeys[(b * plan->nlevels + level) * ORBFE_NK_STRIDE] = n;
    QT_STAMP(2);

    // ---- histogram passes: node-level bookkeeping by the whole workgroup, no key is touched ----
    for (int d = FFD - 1; d >= 1; --d) {  // quadrant sizes of every possible node of depth d-1 .. 4
        const int cntd = nini << (2 * d);
        for (int e = tid; e < cntd; e += QT) {
            const int r = e >> (2 * d), p = e & ((1 << (2 * d)) - 1);
            const int32_t *src = &q.hist[r * FF_PER_ROOT + ff_off(d + 1) + (p << 2)];
            q.hist[r * FF_PER_ROOT + ff_off(d) + p] = src[0] + src[1] + src[2] + src[3];
        }
        __syncthreads();
    }
    if (tid == 0) {  // roots (:545-587): nini boxes, empty roots erased; initial processing order: multi-key roots in list order
        int S0 = 0, m0 = 0;
        for (int r = 0; r < nini; ++r) {
            const int32_t *h1 = &q.hist[r * FF_PER_ROOT];
            const int cn = h1[0] + h1[1] + h1[2] + h1[3];
            if (cn > 0) {
                q.cnt(0)[S0] = cn;
                q.path(0)[S0] = (uint32_t)r << 16;
                if (cn > 1) { q.P[m0] = S0; q.rankOf(0)[S0] = m0; ++m0; }
                else q.rankOf(0)[S0] = -1;
                ++S0;
            }
        }
        misc[0] = S0;
        misc[1] = m0;
    }
    __syncthreads();
    int S = misc[0], m = misc[1], cur = 0, modeB = 0;
    bool finish = false;
    {
        int npass = 0;
        const int ffd = plan->dbg == 50 ? 0 : FFD;  // developer knob: 50 = streaming passes only
        while (!finish && npass < ffd) {  // nodes processed in pass p have depth <= p-1 <= 4: sizes come from the histogram
            if (!modeB && !(plan->dbg == 51)) {  // breadth-first pass (developer knob 51: generic passes only)
                qt_pass_bfs_hist(q, N, S, m, cur, modeB, finish);
                ++npass;
                continue;
            }
            for (int r = tid; r < m; r += QT) {
                const int i = q.P[r];
                const uint32_t pth = q.path(cur)[i];
                const int d = (int)((pth >> 12) & 0xFu), root = (int)(pth >> 16);
                const int32_t *src = &q.hist[root * FF_PER_ROOT + ff_off(d + 1) + (int)((pth & 0xFFFu) << 2)];
                q.cc[i * 4] = src[0];
                q.cc[i * 4 + 1] = src[1];
                q.cc[i * 4 + 2] = src[2];
                q.cc[i * 4 + 3] = src[3];
            }
            __syncthreads();
            qt_node_phase<false>(q, N, S, m, cur, modeB, finish);
            ++npass;
        }
    }
    const bool ff_done = finish;
    QT_STAMP(3);
    // path -> node table of the current list (overwrites the histogram): exactly one node of a key's path exists
    for (int i = tid; i < nini * FF_PER_ROOT; i += QT) q.hist[i] = -1;
    if (tid < ORBFE_MAX_ROOTS) misc[16 + tid] = -1;
    __syncthreads();
    for (int i = tid; i < S; i += QT) {
        const uint32_t pth = q.path(cur)[i];
        const int d = (int)((pth >> 12) & 0xFu), root = (int)(pth >> 16);
        if (d == 0) misc[16 + root] = i;
        else q.hist[root * FF_PER_ROOT + ff_off(d) + (int)(pth & 0xFFFu)] = i;
    }
    __syncthreads();
    // flatten the path -> node table: every leaf learns the one node of its path that exists (the deepest table hit),
    // in place -- a leaf entry is read and written by its own thread only, the shallower levels are read-only here
    for (int i = tid; i < nini << (2 * FFD); i += QT) {
        const int root = i >> (2 * FFD), code = i & ((1 << (2 * FFD)) - 1);
        int idx = misc[16 + root];
#pragma unroll
        for (int d = 1; d < FFD; ++d) {
            const int t = q.hist[root * FF_PER_ROOT + ff_off(d) + (code >> (2 * (FFD - d)))];
            idx = t >= 0 ? t : idx;
        }
        int32_t *leaf = &q.hist[root * FF_PER_ROOT + ff_off(FFD) + code];
        const int t = *leaf;
        *leaf = t >= 0 ? t : idx;
    }
    __syncthreads();
    auto node_of_code = [&](uint32_t kn) { return q.hist[(int)(kn >> 10) * FF_PER_ROOT + ff_off(FFD) + (int)(kn & 0x3FFu)]; };
    QT_STAMP(4);

    if (!ff_done) {
        // ---- deeper trees (clustered candidates): boxes of the current nodes from their paths, keys take their node
        // index, and the passes stream over the keys ----
        for (int i = tid; i < S; i += QT) {
            const uint32_t pth = q.path(cur)[i];
            const int d = (int)((pth >> 12) & 0xFu), root = (int)(pth >> 16);
            int ulx = L.root_x[root], urx = L.root_x[root + 1], uly = 0, bry = ybot;
            for (int s = d - 1; s >= 0; --s) {  // DivideNode along the path (:478-522)
                const int qd = (int)((pth >> (2 * s)) & 3u);
                const int midx = ulx + ((urx - ulx + 1) >> 1), midy = uly + ((bry - uly + 1) >> 1);
                if (qd & 1) ulx = midx; else urx = midx;
                if (qd & 2) uly = midy; else bry = midy;
            }
            q.box(cur, 0)[i] = (int16_t)ulx;
            q.box(cur, 1)[i] = (int16_t)uly;
            q.box(cur, 2)[i] = (int16_t)urx;
            q.box(cur, 3)[i] = (int16_t)bry;
        }
        for (int k = tid; k < ns; k += QT) {
            const uint2 e = SK[k];
            KN[k] = key_kept(e) ? (uint16_t)node_of_code(key_code(e)) : (uint16_t)0xFFFFu;  // 0xFFFF = dropped key
        }
        __syncthreads();
        for (int guard = 0; guard < 64; ++guard) {
            for (int i = tid; i < S * 4; i += QT) q.cc[i] = 0;
            __syncthreads();
            for (int k0 = tid; k0 < ns; k0 += QT * KUNROLL) {
                uint32_t kn[KUNROLL], kv[KUNROLL];
#pragma unroll
                for (int u = 0; u < KUNROLL; ++u) {
                    const int k = min(k0 + u * QT, ns - 1);
                    kn[u] = KN[k];
                    kv[u] = SK[k].x;
                }
#pragma unroll
                for (int u = 0; u < KUNROLL; ++u) {
                    const int k = k0 + u * QT;
                    if (k < ns && kn[u] != 0xFFFFu) {
                        const int i = (int)kn[u];  // node of the current list
                        if (q.cnt(cur)[i] > 1) {
                            const int ulx = q.box(cur, 0)[i], uly = q.box(cur, 1)[i];
                            const int midx = ulx + ((q.box(cur, 2)[i] - ulx + 1) >> 1);  // UL.x + ceil(w/2)  (:480)
                            const int midy = uly + ((q.box(cur, 3)[i] - uly + 1) >> 1);
                            const int qd = (orb_key_x(kv[u]) < midx ? 0 : 1) + (orb_key_y(kv[u]) < midy ? 0 : 2);
                            atomicAdd(&q.cc[i * 4 + qd], 1);
                            KN[k] = (uint16_t)((uint32_t)i | ((uint32_t)qd << 14));
                        }
                    }
                }
            }
            __syncthreads();
            qt_node_phase<true>(q, N, S, m, cur, modeB, finish);
            // keys follow their nodes into the new list (the quadrant counts have just become child positions)
            for (int k = tid; k < ns; k += QT) {
                const uint32_t kn = KN[k];
                if (kn != 0xFFFFu) {
                    const int i = (int)(kn & KNODE_MASK);
                    const int ni = q.newIdx[i];
                    KN[k] = (uint16_t)(ni >= 0 ? ni : q.cc[i * 4 + (int)(kn >> 14)]);
                }
            }
            __syncthreads();
            if (finish) break;
        }
    }

    // ---- keep the strongest key of every node, first in candidate order on ties (:746-762) ----
    // best = response (8 bit) | inverted ord (28 bit: first in candidate order wins ties) | key index (24 bit)
    unsigned long long *best = q.skey;
    for (int i = tid; i < S; i += QT) best[i] = 0ull;
    __syncthreads();
    QT_STAMP(5);
    for (int k0 = tid; k0 < ns; k0 += QT * KUNROLL) {
        uint2 e[KUNROLL];
        uint32_t kn[KUNROLL];
#pragma unroll
        for (int u = 0; u < KUNROLL; ++u) {
            const int k = min(k0 + u * QT, ns - 1);
            e[u] = SK[k];
            kn[u] = ff_done ? 0u : (uint32_t)KN[k];
        }
#pragma unroll
        for (int u = 0; u < KUNROLL; ++u) {
            const int k = k0 + u * QT;
            if (k < ns && (ff_done ? key_kept(e[u]) : kn[u] != 0xFFFFu)) {
                const int i = ff_done ? node_of_code(key_code(e[u])) : (int)kn[u];
                const unsigned long long cand = ((unsigned long long)orb_key_r(e[u].x) << 52) |
                                                ((unsigned long long)(0x0FFFFFFFu - e[u].y) << 24) | (unsigned long long)k;
                // neighbouring keys share nodes: a plain read filters most of them before the (serialising) atomic
                if (cand > best[i]) atomicMax(&best[i], cand);
            }
        }
    }
    __syncthreads();
    QT_STAMP(6);
    uint32_t *out = sel + (int64_t)b * plan->sel_per_frame + L.sel_off;
    const int nout = min(S, L.sel_cap);
    for (int i = tid; i < nout; i += QT) {
        const uint32_t key = SK[(uint32_t)(best[i] & 0xFFFFFFull)].x;
        // + minBorderX / minBorderY (:853-854): level coordinates from here on
        out[i] = orb_pack_key(orb_key_x(key) + ORBFE_MINB, orb_key_y(key) + ORBFE_MINB, orb_key_r(key));
    }
    if (tid == 0) {
        nsel[b * plan->nlevels + level] = nout;
        if (S > L.sel_cap) atomicOr(ovf, 2);
    }
    QT_STAMP(7);
}

// ---------------------------------------------------------------------------------------------------
// launchers (host)
// ---------------------------------------------------------------------------------------------------
hipError_t orbk_launch_octree(const OrbLaunch &a, hipStream_t st)
{
    // Level groups [0, nl/8), [nl/8, nl/2), [nl/2, nl) with 512 / 256 / 128 threads: the geometric feature split gives
    // level 0 about 3.6x the features (and many times the candidates) of level 7.  Measured per 1024 frames of 640x480 /
    // 1000 features: one launch of 512-thread workgroups 0.385 ms (dense-corner frames S) / 0.39 ms (camera-like frames
    // S_tum); this grouping 0.335 / 0.28 ms; {1,4,8} x 256 threads 0.33 / 0.315; four or more groups are slower again
    // (every launch has its own tail).
    const OrbPlan &P = *a.h_plan;
    const int nl = P.nlevels;
    // Small batches do not fill the chip: there the launches would only add their latencies (a workgroup's serial
    // bookkeeping, ~45 us each: single-frame host latency 0.26 -> 0.35 ms), so they take one launch.
    const bool grouped = a.nframes >= 128;
    const int cut[4] = {0, grouped ? std::max(1, nl / 8) : nl, grouped ? std::max(1, nl / 2) : nl, nl};
    int qts[3] = {512, 256, 128};
    for (int i = 0; i < 3; ++i)   // ORBFE_OPT_QT_THREADS_0..2: threads per workgroup of the three level groups
        if (a.opts.qt[i] >= 64 && a.opts.qt[i] <= QT_MAX && a.opts.qt[i] % 64 == 0) qts[i] = a.opts.qt[i];
    for (int gi = 0; gi < 3; ++gi) {
        const int l0 = cut[gi], l1 = std::min(cut[gi + 1], nl);
        if (l1 <= l0) continue;
        OctGroup g;
        g.level0 = l0;
        g.M = 64; g.nini = 1; g.tw = 2; g.th = 2; g.ncells = 1;
        for (int l = l0; l < l1; ++l) {
            const OrbLevel &L = P.lv[l];
            g.M = std::max(g.M, (int)orb_align_up(L.sel_cap + 1, 64));
            g.nini = std::max(g.nini, (int)L.nini);
            g.tw = std::max(g.tw, (int)L.w);
            g.th = std::max(g.th, (int)L.h);
            g.ncells = std::max(g.ncells, (int)L.ncells);
        }
        const size_t lds = orbk_octree_lds_bytes(g.M, g.nini, g.tw, g.th, g.ncells);
        const int qt = qts[gi];
        if (lds <= (size_t)ORBFE_LDS_MAX)
            hipLaunchKernelGGL(k_octree<false>, dim3(l1 - l0, a.nframes), dim3(qt), lds, st, a.d_plan, a.d_skeys, a.d_scount, a.d_cflag,
                               a.cf_words, a.d_knode, a.d_qtbox, a.qtbox_stride, (char *)nullptr, (int64_t)0, a.d_nkeys, a.d_sel, a.d_nsel,
                               a.d_ovf, g);
        else  // more nodes than the LDS holds: node arrays in the global scratch slice of each (frame, level)
            hipLaunchKernelGGL(k_octree<true>, dim3(l1 - l0, a.nframes), dim3(QT_MAX), octree_table_bytes(g.nini, g.tw, g.th, g.ncells), st,
                               a.d_plan, a.d_skeys, a.d_scount, a.d_cflag, a.cf_words, a.d_knode, a.d_qtbox, a.qtbox_stride, a.d_qtnodes,
                               a.qtnodes_stride, a.d_nkeys, a.d_sel, a.d_nsel, a.d_ovf, g);
    }
    return hipGetLastError();
}

hipError_t orbk_prepare_octree(int node_cap, int max_nini, int w, int h, int ncells)
{
    // The attribute is per kernel and process-wide: every handle sets it to the SAME value, the most the code can ever
    // request (the CU's 160 KB), so a later, smaller handle can never lower the limit under an earlier, larger one.
    (void)node_cap;
    if (octree_table_bytes(max_nini, w, h, ncells) > (size_t)ORBFE_LDS_MAX) return hipErrorInvalidValue;
    hipError_t e = hipFuncSetAttribute((const void *)k_octree<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ORBFE_LDS_MAX);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute((const void *)k_octree<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ORBFE_LDS_MAX);
}
