// orbfe_matcher.h -- the matcher handle, shared by the translation units that implement its entry points (orbfe_match.hip,
// orbfe_grid.hip, orbfe_projection.hip, orbfe_track.hip, orbfe_init_search.hip, orbfe_tri_search.hip, orbfe_stereo.hip, orbfe_bow.hip, orbfe_frame.hip) and by orbfe_pipeline.hip,
// with what more than one of them does to it: the scratch hand-over between streams, the pinned input staging (stage_upload) and
// the check of a caller's grid (orb_grid_csr_ok).  Host only; the device side the projection searches share is orbfe_proj_dev.h.
#pragma once

#include "orbfe_common.h"
#include "orbfe_host.h"

struct orbfe_matcher {
    int device = 0;
    hipStream_t stream = nullptr;
    DevBuf b[16];
    bool own_stream = true;  // false: the stream belongs to a pipeline (orbfe_internal_matcher_create_on_stream)
    int bf_kernel = 0;  // 0 = k_match_bf (FP4 dot product on the matrix cores), 1 = k_match_popc (xor / popcount)
    int bf_tiles = 4;   // query tiles per wave of k_match_bf: 4, 2 or 1 (orbfe_internal_matcher_set_bf_tiles)
    // Device entry points that use the scratch blocks b[] run on the CALLER's stream: one that arrives on another stream
    // than its predecessor waits (at stream level) for the event recorded behind that predecessor's last launch.
    hipStream_t scratch_stream = nullptr;
    bool scratch_used = false;
    hipEvent_t ev_scratch = nullptr;
    PinBuf pin_in, pin_out;  // page-locked staging of the latency-bound per-frame calls (orbfe_search_by_projection)
    bool proj_fused = true;   // orbfe_search_by_projection: the one-launch form (k_proj_fused); false = the four-kernel path (tests)
    int tri_kernel = 0;       // orbfe_search_for_triangulation_batch_device: 0 = k_tri_search (LDS tiles), 1 = k_tri_search_flat
    DevBuf proj_done;        // k_proj_fused's arrival counter / overflow word (zero between calls)
    orbfe_matcher()
    {
        for (DevBuf &x : b) x.min_bytes = 4;
        proj_done.min_bytes = pin_in.min_bytes = pin_out.min_bytes = 4;
        pin_in.slack = pin_out.slack = true;
    }
};

static inline hipError_t scratch_acquire(orbfe_matcher *m, hipStream_t st)
{
    if (m->scratch_used && m->scratch_stream != st) return hipStreamWaitEvent(st, m->ev_scratch, 0);
    return hipSuccess;
}
static inline hipError_t scratch_release(orbfe_matcher *m, hipStream_t st)
{
    m->scratch_stream = st;
    m->scratch_used = true;
    return hipEventRecord(m->ev_scratch, st);
}

// The input staging of the latency-bound host-buffer calls (one pageable copy per array costs more than their kernels): the N
// pieces are packed into pin_in at 256-byte aligned offsets in list order, go to b[0] in ONE upload on `st`, and dev[i] is the
// device address of piece i.  A piece of 0 bytes takes no room and is not copied; its address is not to be used.
struct StagePiece {
    const void *src;
    size_t bytes;
    const void *src2 = nullptr;   // a second array right behind the first, in the same piece
    size_t bytes2 = 0;
};
template <int N>
static inline hipError_t stage_upload(orbfe_matcher *m, hipStream_t st, const StagePiece (&piece)[N], const char *(&dev)[N])
{
    size_t at[N + 1];
    at[0] = 0;
    for (int i = 0; i < N; ++i) at[i + 1] = orb_align256(at[i] + piece[i].bytes + piece[i].bytes2);
    hipError_t e = m->pin_in.ensure(at[N]);
    if (e == hipSuccess) e = m->b[0].ensure(at[N]);
    if (e != hipSuccess) return e;
    for (int i = 0; i < N; ++i) {
        if (piece[i].bytes) memcpy(m->pin_in.as<char>() + at[i], piece[i].src, piece[i].bytes);
        if (piece[i].bytes2) memcpy(m->pin_in.as<char>() + at[i] + piece[i].bytes, piece[i].src2, piece[i].bytes2);
        dev[i] = m->b[0].as<const char>() + at[i];
    }
    return hipMemcpyAsync(m->b[0].p, m->pin_in.p, at[N], hipMemcpyHostToDevice, st);
}

// A caller's grid in CSR form (cell_off[cells + 1], cell_idx[cell_off[cells]]) over n features: false, with the error text
// set, when a kernel could leave the arrays through it.  `n_name` is the name of n in the caller's argument list.
static inline bool orb_grid_csr_ok(const uint32_t *cell_off, const uint32_t *cell_idx, int32_t n, const char *n_name)
{
    const int nc = ORBFE_GRID_COLS * ORBFE_GRID_ROWS;
    const uint32_t nin = cell_off[nc];
    if (nin > (uint32_t)n) { orbfe_set_error("cell_off inconsistent with %s", n_name); return false; }
    for (int c = 0; c < nc; ++c)
        if (cell_off[c + 1] < cell_off[c]) { orbfe_set_error("cell_off must not decrease"); return false; }
    for (uint32_t k = 0; k < nin; ++k)
        if (cell_idx[k] >= (uint32_t)n) { orbfe_set_error("cell_idx out of range"); return false; }
    return true;
}

// a matcher for a pipe of orbfe_pipeline: `st` (the pipe's stream) is its own stream and stays the pipeline's
orbfe_status orbfe_internal_matcher_create_on_stream(int32_t device, void *st, orbfe_matcher **out);

// the instantiations of k_match_bf (orbfe_match.hip): query tiles per wave
static inline bool orb_match_tiles_ok(int32_t tiles) { return tiles == 4 || tiles == 2 || tiles == 1; }
// orbfe_match_bf_blocks_device with the tile count of the call instead of the handle's
orbfe_status orbfe_internal_match_bf_blocks_tiles(orbfe_matcher *m, const orbfe_keypoint *d_qkps, const uint8_t *d_qdesc, const int32_t *d_qn,
                                                  const orbfe_keypoint *d_tkps, const uint8_t *d_tdesc, const int32_t *d_tn, int32_t cap,
                                                  const int32_t *d_qframe, const int32_t *d_tframe, int32_t npairs, float nnratio, int32_t th,
                                                  int32_t check_ori, int32_t *d_match_q2t, int32_t *d_nmatches, int32_t tiles, void *stream);

// single-workgroup exclusive scan cnt[0..nq) -> off[0..nq] on `st`: k_scan_u32 lives in orbfe_grid.hip and this is its one launch
// site, for the grid's own entry points and for orbfe_projection.hip (not exported)
__attribute__((visibility("hidden"))) void orbfe_internal_launch_scan_u32(const uint32_t *cnt, int nq, uint32_t *off, hipStream_t st);
