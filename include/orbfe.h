/*
 * orbfe.h -- C-ABI of the MI355X-native ORB front-end (liborbfe.so).
 *
 * Drop-in boundary for ONE hot path of Ewenwan/ORB_SLAM2_SSD_Semantic:
 *   ORB_SLAM2::ORBextractor::operator()      (reference include/ORBextractor.h:53-55, src/ORBextractor.cc:1052)
 *   ORB_SLAM2::ORBmatcher Hamming core        (reference include/ORBmatcher.h:41-112, src/ORBmatcher.cc)
 * The reference has no FFI: the "operator API" is two C++ classes.  The C++ shim in
 * orb_slam2_ssd_semantic_amd/shim/ re-declares those classes with identical signatures on top of
 * this header (INTEGRATION.md shows the binding).  Plain C, POD only, caller-owned buffers, every
 * call returns an orbfe_status (0 = ok, negative = error); nothing throws or aborts.
 *
 * Threading: a handle is used by one thread at a time (like an ORBextractor instance, which mutates
 * mvImagePyramid); different handles may be used concurrently (stereo: src/Frame.cc:121-122;
 * matchers are created per call site from three SLAM threads).  There is no global
 * mutable state.
 *
 * All compute runs in hand-written HIP kernels for gfx950.  There is NO CPU fallback: without a
 * usable HIP device orbfe_create / orbfe_matcher_create fail with ORBFE_ERR_NODEVICE.
 */
#ifndef ORBFE_H
#define ORBFE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBFE_VERSION 100 /* 0.1.0 */

typedef int32_t orbfe_status;
enum {
    ORBFE_OK = 0,
    ORBFE_ERR_ARG = -1,      /* null pointer / negative size / inconsistent arguments          */
    ORBFE_ERR_SIZE = -2,     /* image larger than planned or too small for the 8-level grid    */
    ORBFE_ERR_CAP = -3,      /* caller's keypoint capacity too small; *n_out holds the need    */
    ORBFE_ERR_HIP = -4,      /* a HIP runtime call failed (see orbfe_last_error)               */
    ORBFE_ERR_NOMEM = -5,    /* device or host allocation failed                               */
    ORBFE_ERR_NODEVICE = -6, /* no usable HIP device: there is no CPU path                     */
    ORBFE_ERR_STATE = -7     /* call made in the wrong state (e.g. taps before any extract)    */
};

/* = cv::KeyPoint field order (T1): {Point2f pt; float size, angle, response; int octave, class_id}. 28 B. */
typedef struct orbfe_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} orbfe_keypoint;

/* Constructor arguments of ORBextractor (include/ORBextractor.h:45-46, values read from the settings
 * YAML at src/Tracking.cc:198-206) plus planning sizes for the device buffers. */
typedef struct orbfe_params {
    int32_t nfeatures;      /* ORBextractor.nFeatures   (TUM3.yaml:41-54: 1000) */
    float scale_factor;     /* ORBextractor.scaleFactor (1.2)                   */
    int32_t nlevels;        /* ORBextractor.nLevels     (8), 1..16              */
    int32_t ini_th_fast;    /* ORBextractor.iniThFAST   (20)                    */
    int32_t min_th_fast;    /* ORBextractor.minThFAST   (7)                     */
    int32_t max_width;      /* largest image width this handle will see  (<= 4096) */
    int32_t max_height;     /* largest image height this handle will see (<= 4096) */
    int32_t max_batch;      /* frames per batched call (>= 1)                   */
    int32_t device;         /* HIP device ordinal, -1 = current device          */
    int32_t blur_rounding;  /* 0 = canonical half-up; 1 = emulate the x86 SSE2 column kernel */
} orbfe_params;

typedef struct orbfe_handle orbfe_handle;   /* one ORBextractor instance */
typedef struct orbfe_matcher orbfe_matcher; /* scratch + stream for ORBmatcher calls */

/* ---------------------------------------------------------------------------------------------
 * Library
 * ------------------------------------------------------------------------------------------- */
int32_t orbfe_version(void);
const char *orbfe_strerror(orbfe_status s);
/* thread-local text of the last failure on the calling thread ("" if none) */
const char *orbfe_last_error(void);
/* number of visible HIP devices (0 when there is none; never fails) */
int32_t orbfe_device_count(void);

/* ---------------------------------------------------------------------------------------------
 * Extractor  (replaces ORBextractor: ctor src/ORBextractor.cc:399-466, operator() :1052-1114)
 * ------------------------------------------------------------------------------------------- */
/* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST) */
orbfe_status orbfe_create(const orbfe_params *p, orbfe_handle **out);
void orbfe_destroy(orbfe_handle *h);

/* GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares / GetInverseScaleSigmaSquares
 * (include/ORBextractor.h:58-78); nlevels floats each, any pointer may be NULL. */
orbfe_status orbfe_get_scales(const orbfe_handle *h, float *scale, float *inv_scale, float *sigma2,
                              float *inv_sigma2);
/* mnFeaturesPerLevel (src/ORBextractor.cc:426-439); nlevels ints */
orbfe_status orbfe_get_features_per_level(const orbfe_handle *h, int32_t *out);
/* upper bound of keypoints one frame can produce: sum over levels of max(N_l + 2, 4 * nIni_l) -- the quadtree may end
 * a pass with up to 3 nodes more than asked, and never with fewer than the initial roots' children -- rounded up to 64 */
int32_t orbfe_keypoint_capacity(const orbfe_handle *h);

/* ORBextractor::operator()(image, mask, keypoints, descriptors) for one 8-bit gray frame in HOST
 * memory (mask is ignored by the reference, :1052).  kps/desc are caller-owned with room for `cap`
 * keypoints; *n_out receives the count.  w==0 || h==0 || gray==NULL -> ORBFE_OK, outputs untouched
 * (:1055-1056).  Order of the output is the reference's (level-major, quadtree list order). */
orbfe_status orbfe_extract(orbfe_handle *h, const uint8_t *gray, int32_t w, int32_t ht, int32_t stride,
                           orbfe_keypoint *kps, uint8_t *desc /* cap x 32 */, int32_t cap, int32_t *n_out);

/* Batched keyframe mode, HOST buffers: frames are independent.  grays[i] points to
 * frame i (all w x ht, same stride).  Frame i writes kps[i*cap ..], desc[i*cap*32 ..], n_out[i].
 * More than max_batch frames run as a pipeline (H2D of the next chunk, kernels of the current one and D2H of the previous
 * one overlap on three streams).  Page-locked memory (hipHostMalloc / hipHostRegister / torch pin_memory) is used as it
 * is: frames with stride == w are copied straight from the caller's buffers, and page-locked kps / desc / n_out arrays
 * receive the padded device blocks directly (slots >= n_out[i] zero-filled); pageable memory goes through the handle's
 * own pinned staging sets. */
orbfe_status orbfe_extract_batch(orbfe_handle *h, const uint8_t *const *grays, int32_t nframes, int32_t w,
                                 int32_t ht, int32_t stride, orbfe_keypoint *kps, uint8_t *desc, int32_t cap,
                                 int32_t *n_out);

/* Batched keyframe mode, DEVICE buffers (HBM-resident input, what bench.py times):
 *   d_gray   : nframes frames, frame i at d_gray + i*frame_stride, row pitch `stride`; nothing outside
 *              [d_gray, last pixel of the last frame] is read (row windows are pulled back at the right edge)
 *   d_kps    : nframes*cap orbfe_keypoint      d_desc : nframes*cap*32 bytes     d_n_out : nframes int32
 * All work is enqueued on `stream`, a hipStream_t passed as void*.  NULL is HIP's (legacy) default stream
 * -- the stream PyTorch uses unless told otherwise; pass orbfe_get_stream(h) for the handle's own
 * non-blocking stream.  The call returns without synchronising.  Slots >= n_out[i] of a frame are zero-filled so the
 * padded buffers can be all-gathered as they are.
 * Lifetime: level 0 of the pyramid is read IN PLACE from d_gray, also by later orbfe_get_pyramid_level /
 * orbfe_tap_* / orbfe_stereo_matches calls on this handle -- keep d_gray alive and unchanged until the next extract
 * call (or until you are done with those calls).  With the host entry points only the frames of the last chunk of
 * max_batch frames stay addressable. */
orbfe_status orbfe_extract_batch_device(orbfe_handle *h, const uint8_t *d_gray, int32_t nframes, int32_t w,
                                        int32_t ht, int32_t stride, size_t frame_stride,
                                        orbfe_keypoint *d_kps, uint8_t *d_desc, int32_t cap,
                                        int32_t *d_n_out, void *stream);
/* Capacity check for the DEVICE entry point (the host entry points do it themselves and return ORBFE_ERR_CAP):
 * every internal list is sized for its worst case, and the kernels raise a sticky device-side word instead of
 * silently dropping data if a size is ever exceeded.  Waits for the stream of the last batched call, returns and
 * clears the word: bit 0 = a level's FAST survivor list overflowed, bit 1 = a level's quadtree selection overflowed,
 * bit 2 = a frame produced more keypoints than `cap` (d_n_out holds the required count). */
orbfe_status orbfe_get_overflow(orbfe_handle *h, int32_t *flags);
/* FAST kernel variant.  Results are identical in every mode.
 *   0  dense: the 16 nine-arcs of every pixel
 *   1  dense with wave-uniform shortcuts (skips the arc evaluation of 256-pixel row pieces that fail a 4-point necessary
 *      test, and the suppression of rows without strength)
 *   2  lane-compacting: every pixel pair takes the 4-point necessary test; the pairs that pass leave a tag in a queue and are
 *      evaluated, 64 at a time, one per lane, from a ring of the pixel rows the wave holds in LDS -- cheaper than dense when few
 *      pairs pass (FAST stage of 1024 frames of 640x480: -16 % at the 18 % of the camera-like synthetic frames S_tum, -28 % at
 *      8 %, -40 % at 2 %; break-even near 27 %), dearer when more do (+45 % at the 84 % of the corner-saturated frames S), and
 *      dearer for calls that do not fill the GPU (its waves are longer: +15 % on one frame)
 *   3  auto (the default): 0 for calls that do not fill the GPU (less work than about 29 frames of 640x480); otherwise 2, and 0 for the next 16 calls (doubling up to 256 while
 *      it keeps happening) whenever the compacting kernel reported more than 25 % passing pairs
 * collect_stats != 0 counts {row steps, arc skips, NMS skips} (mode 1) / {row steps, batches, parked pairs} of a sample of the
 * waves (mode 2); in mode 3 orbfe_get_fast_stats returns the counters of the last probe that completed (zeros before one has). */
orbfe_status orbfe_set_fast_mode(orbfe_handle *h, int32_t mode, int32_t collect_stats);
orbfe_status orbfe_get_fast_stats(orbfe_handle *h, uint64_t out[3], int32_t reset);
/* work model of the FAST kernel for the current frame size: out[0] = wave row steps per frame (one step = 64 lanes x 4
 * pixels of one row, halo rows included), out[1] = waves per frame.  bench.py prices its VALU ceiling with it. */
orbfe_status orbfe_get_work_counts(const orbfe_handle *h, int64_t out[2]);
/* Launch-shape and A/B options of a handle.  The release library takes them ONLY through this call -- it reads no tuning
 * knob from the process environment (a library inside a SLAM process must not change algorithm because of the host's
 * environment).  Every setting gives byte-identical results (ORBFE_OPT_BLUR_ROUNDING excepted).  Built-in choices, i.e. the value that
 * restores the default: OVERLAP -1; ROWS / ROWS_FAST / ROWS_BLUR / PYR_ROWS / QT_THREADS_* 0; BLUR_PIECES 1 (0 = the older packing, an
 * A/B variant); BLUR_UPDOWN 1 (0 = never, 2 = always); DEBUG 0; REUSE_IDENTICAL_INPUT 0.
 * A developer build (-DORBFE_DEVELOPER, tools/ab_build.sh) also honours $ORBFE_<NAME> at orbfe_create.  The numbers 12 .. 15
 * belonged to kernel variants that were measured slower than the default and have been removed; they stay reserved: value 0
 * is accepted, anything else answers ORBFE_ERR_ARG.  Call between extract calls, not concurrently with one. */
enum {
    ORBFE_OPT_OVERLAP = 1,        /* blur on the side stream: 0 never, 1 from before FAST, 2 beside the quadtree, -1 by batch size */
    ORBFE_OPT_ROWS = 2,           /* rows a FAST / blur wave walks (8..512) */
    ORBFE_OPT_ROWS_FAST = 3,      /* ... FAST only */
    ORBFE_OPT_ROWS_BLUR = 4,      /* ... blur only */
    ORBFE_OPT_BLUR_PIECES = 5,    /* 1 (default): blur lanes laid out in 64-byte pieces */
    ORBFE_OPT_BLUR_UPDOWN = 6,    /* odd row blocks of the blur walk upwards: 0 never, 1 where it adds no wave (default), 2 always */
    ORBFE_OPT_PYR_ROWS = 7,       /* destination rows per lane run of the pyramid kernel (2..16) */
    ORBFE_OPT_QT_THREADS_0 = 8,   /* threads per workgroup of the quadtree's three level groups (64..512, multiple of 64) */
    ORBFE_OPT_QT_THREADS_1 = 9,
    ORBFE_OPT_QT_THREADS_2 = 10,
    ORBFE_OPT_DEBUG = 11,         /* forces production code paths that ordinary frames rarely take (tests): 50 = quadtree by
                                   * streaming key passes only (the deep-tree path), 51 = generic node passes only */
    /* 12 .. 15: retired, reserved */
    ORBFE_OPT_BLUR_ROUNDING = 16, /* orbfe_params.blur_rounding of an existing handle (0 / 1); this one changes RESULTS */
    ORBFE_OPT_REUSE_IDENTICAL_INPUT = 17 /* single-frame host calls (orbfe_extract; orbfe_extract_batch with one frame), default 0.  1: a call whose
                                   * pixels equal those of the previous such call of this handle (same w, ht, cap; compared on the host against the pinned
                                   * staging copy, stride-independent) returns that call's keypoints / descriptors without
                                   * touching the GPU; pyramid and taps stay those of that frame.  For callers that extract the
                                   * same image twice: perfect/src/Tracking.cc:685 and :716 build two Frames from one mImGray.
                                   * Bit-exact by construction.  Any other use of the handle in between drops the cached frame. */
};
orbfe_status orbfe_set_option(orbfe_handle *h, int32_t option, int32_t value);
/* 1 when the last orbfe_extract call of the handle was answered from the previous call's results (ORBFE_OPT_REUSE_IDENTICAL_INPUT) */
int32_t orbfe_last_call_reused(const orbfe_handle *h);
/* the handle's own non-blocking stream (hipStream_t as void*): the host-buffer entry points run on it */
void *orbfe_get_stream(orbfe_handle *h);
/* block until everything enqueued by this handle on its own stream has finished */
orbfe_status orbfe_synchronize(orbfe_handle *h);

/* mvImagePyramid[level] of the LAST extract call, frame `frame` of the batch (include/ORBextractor.h:80;
 * read by Frame::ComputeStereoMatches src/Frame.cc:649,761-778).  with_border != 0 returns the
 * (w+38) x (h+38) BORDER_REFLECT_101-padded image (src/ORBextractor.cc:1136-1142), else w x h. */
orbfe_status orbfe_get_level_size(const orbfe_handle *h, int32_t level, int32_t *w, int32_t *ht);
orbfe_status orbfe_get_pyramid_level(orbfe_handle *h, int32_t frame, int32_t level, uint8_t *dst,
                                     int32_t dst_stride, int32_t with_border);
/* The same for ALL levels in one go -- the public mvImagePyramid of the reference (src/ORBextractor.cc:1128-1142): level l of
 * frame `frame` with its 19-px BORDER_REFLECT_101 frame as a (w_l + 38) x (h_l + 38) block with tight rows (pitch w_l + 38)
 * at offsets[l] of dst (blocks back to back, each offset a multiple of 64); *total = bytes needed.  dst == NULL: sizes only.
 * One kernel + ONE device-to-host copy (dst may be pageable).  offsets [nlevels] and total may be NULL. */
orbfe_status orbfe_get_pyramid_padded(orbfe_handle *h, int32_t frame, uint8_t *dst, size_t cap, size_t *offsets, size_t *total);

/* ---- stage taps of the last extract call (parity tests / debugging; host copies) ---- */
/* 7x7 sigma-2 blurred level (the private clone of src/ORBextractor.cc:1094-1095) */
orbfe_status orbfe_tap_blurred_level(orbfe_handle *h, int32_t frame, int32_t level, uint8_t *dst,
                                     int32_t dst_stride);
/* FAST candidates handed to DistributeOctTree for one level, reference order (cell-row-major, raster):
 * xyr = n x {x, y, response} floats in detection-window coordinates (src/ORBextractor.cc:831-833) */
orbfe_status orbfe_tap_candidates(orbfe_handle *h, int32_t frame, int32_t level, float *xyr, int32_t cap,
                                  int32_t *n);
/* keypoints kept by DistributeOctTree for one level, list order, level coordinates (border added) */
orbfe_status orbfe_tap_selected(orbfe_handle *h, int32_t frame, int32_t level, float *xyr, int32_t cap,
                                int32_t *n);

/* ---- timing of the last batched call (HIP events on the stream the kernels ran on) ---- */
enum {
    ORBFE_T_PYRAMID = 0, /* all resize launches                                  */
    ORBFE_T_FAST = 1,    /* FAST score + per-cell NMS + threshold fallback       */
    ORBFE_T_OCTREE = 2,  /* DistributeOctTree                                    */
    ORBFE_T_BLUR = 3,    /* 7x7 Gaussian                                         */
    ORBFE_T_DESC = 4,    /* IC_Angle + rBRIEF + keypoint assembly                */
    ORBFE_T_TOTAL = 5,   /* first launch -> last launch                          */
    ORBFE_T_COUNT = 6
};
/* enable != 0: record events around each stage of subsequent calls (adds a few us per call) and reset
 * the averaging window */
orbfe_status orbfe_set_profiling(orbfe_handle *h, int32_t enable);
/* milliseconds per stage, AVERAGED over the calls made since profiling was enabled (the 64 most recent at
 * most); waits for those calls to finish */
orbfe_status orbfe_get_stage_ms(orbfe_handle *h, float ms[ORBFE_T_COUNT]);

/* ---------------------------------------------------------------------------------------------
 * Matcher  (replaces the Hamming core of ORBmatcher, src/ORBmatcher.cc)
 * ------------------------------------------------------------------------------------------- */
#define ORBFE_TH_HIGH 100     /* ORBmatcher::TH_HIGH      src/ORBmatcher.cc:39 */
#define ORBFE_TH_LOW 50       /* ORBmatcher::TH_LOW       src/ORBmatcher.cc:40 */
#define ORBFE_HISTO_LENGTH 30 /* ORBmatcher::HISTO_LENGTH src/ORBmatcher.cc:41 */

/* ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1968-1984): host scalar, no device involved */
int32_t orbfe_hamming(const uint8_t a[32], const uint8_t b[32]);

orbfe_status orbfe_matcher_create(int32_t device /* -1 = current */, orbfe_matcher **out);
void orbfe_matcher_destroy(orbfe_matcher *m);

/* BASELINE config 3 "brute-force Hamming match to previous frame" (SURVEY 8(a) M3): for every query
 * row the best / second-best distance over ALL train rows with the update idiom of
 * src/ORBmatcher.cc:280-289 (ties: lowest train index), accepted when best <= th and
 * (float)best < nnratio*(float)second, then the rotation-consistency histogram (:308-316, :338-360,
 * ComputeThreeMaxima :1912-1957) when check_ori != 0.  HOST buffers.
 *   match_q2t[nq] : train index or -1        best/second[nq] : may be NULL        *nmatches : kept */
orbfe_status orbfe_match_bf(orbfe_matcher *m, const uint8_t *q, int32_t nq, const uint8_t *t, int32_t nt,
                            const float *q_angle, const float *t_angle, float nnratio, int32_t th,
                            int32_t check_ori, int32_t *match_q2t, int32_t *best, int32_t *second,
                            int32_t *nmatches);
void *orbfe_matcher_get_stream(orbfe_matcher *m);
/* all-pairs kernel behind the three orbfe_match_bf* calls: 0 (default) = exact FP4 dot product on the matrix cores
 * (every bit a +-1, dot = 256 - 2 * hamming, v_mfma_scale_f32_32x32x64_f8f6f4), 1 = xor / popcount.  Results are identical; see DESIGN.md for the measured A/B. */
orbfe_status orbfe_matcher_set_bf_kernel(orbfe_matcher *m, int32_t kernel);
/* orbfe_search_by_projection(_chi2): 0 (default) = the whole search in ONE launch (k_proj_fused: per-query slabs, round 0 of the
 * relaxation decided while the candidates are written, the last workgroup finishes the rounds, results stored straight into
 * page-locked host memory), falling back to 1 = count -> scan -> fill -> resolve when a query has more than 512 candidates or
 * the tables exceed 64 KB of LDS.  Identical results. */
orbfe_status orbfe_matcher_set_projection_kernel(orbfe_matcher *m, int32_t kernel);
/* same, DEVICE buffers, enqueued on `stream` (NULL = HIP's default stream, see orbfe_extract_batch_device;
 * orbfe_matcher_get_stream(m) = the matcher's own stream), no synchronisation;
 * d_nmatches is one int32 in device memory */
orbfe_status orbfe_match_bf_device(orbfe_matcher *m, const uint8_t *d_q, int32_t nq, const uint8_t *d_t,
                                   int32_t nt, const float *d_q_angle, const float *d_t_angle, float nnratio,
                                   int32_t th, int32_t check_ori, int32_t *d_match_q2t, int32_t *d_best,
                                   int32_t *d_second, int32_t *d_nmatches, void *stream);
/* batched form of the above: pair p matches frame p (queries) against frame p+1's predecessor layout:
 *   queries  = d_desc + qframe[p]*cap*32 (nq = d_n[qframe[p]]),  train = d_desc + tframe[p]*cap*32
 * with angles taken from d_kps (orbfe_keypoint.angle).  Outputs are npairs x cap. Used by bench.py. */
orbfe_status orbfe_match_bf_frames_device(orbfe_matcher *m, const orbfe_keypoint *d_kps, const uint8_t *d_desc,
                                          const int32_t *d_n, int32_t cap, const int32_t *d_qframe,
                                          const int32_t *d_tframe, int32_t npairs, float nnratio, int32_t th,
                                          int32_t check_ori, int32_t *d_match_q2t /* npairs*cap */,
                                          int32_t *d_nmatches /* npairs */, void *stream);

/* the same with queries and train frames taken from two DIFFERENT output blocks of the same `cap` (e.g. the frames of this
 * batch against frames of the previous batch): d_qframe indexes (d_qkps, d_qdesc, d_qn), d_tframe indexes (d_tkps, d_tdesc, d_tn) */
orbfe_status orbfe_match_bf_blocks_device(orbfe_matcher *m, const orbfe_keypoint *d_qkps, const uint8_t *d_qdesc,
                                          const int32_t *d_qn, const orbfe_keypoint *d_tkps, const uint8_t *d_tdesc,
                                          const int32_t *d_tn, int32_t cap, const int32_t *d_qframe, const int32_t *d_tframe,
                                          int32_t npairs, float nnratio, int32_t th, int32_t check_ori,
                                          int32_t *d_match_q2t /* npairs*cap */, int32_t *d_nmatches /* npairs */, void *stream);

/* ORBmatcher::SearchByBoW (KeyFrame*, Frame&, ...) src/ORBmatcher.cc:217-363   [strict_lt = 0, validF = NULL]
 * ORBmatcher::SearchByBoW (KeyFrame*, KeyFrame*, ...) src/ORBmatcher.cc:665-812 [strict_lt = 1]
 * DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned>>) is passed as CSR: node[nnodes] ascending,
 * off[nnodes+1], idx[off[nnodes]].  Each feature index must occur in at most one node (true for
 * FeatureVectors produced by DBoW2 transform()); otherwise ORBFE_ERR_ARG.
 *   validKF[nKF] : 1 where the KF feature has a good MapPoint (pMP && !pMP->isBad()), NULL = all
 *   validF[nF]   : same for the second keyframe (M2), NULL for a Frame (M1)
 *   matchF2KF[nF]: KF feature index whose MapPoint is assigned to F feature i, -1 = none
 * HOST buffers. */
orbfe_status orbfe_search_by_bow(orbfe_matcher *m, const uint8_t *descKF, int32_t nKF, const uint8_t *validKF,
                                 const float *angKF, const uint32_t *nodeKF, const uint32_t *offKF,
                                 const uint32_t *idxKF, int32_t nnodesKF, const uint8_t *descF, int32_t nF,
                                 const uint8_t *validF, const float *angF, const uint32_t *nodeF,
                                 const uint32_t *offF, const uint32_t *idxF, int32_t nnodesF, float nnratio,
                                 int32_t th_low, int32_t strict_lt, int32_t check_ori, int32_t *matchF2KF,
                                 int32_t *nmatches);

/* batched best / second-best over per-query candidate lists (CSR), the inner loop of the
 * SearchByProjection / SearchForTriangulation / SearchBySim3 / Fuse family (src/ORBmatcher.cc:63,378,827,
 * 1031,1198,1334,1578,1757): the pose/grid gating stays on the host, the Hamming work comes here.
 * best_idx[nq] = candidate (train row) with the minimum distance, first in list order on ties, -1 if
 * the list is empty; best/second initialised to 256.  HOST buffers. */
orbfe_status orbfe_hamming_csr(orbfe_matcher *m, const uint8_t *q, int32_t nq, const uint8_t *t, int32_t nt,
                               const uint32_t *off, const uint32_t *cand, int32_t *best_idx, int32_t *best,
                               int32_t *second);
/* same, plus second_idx[nq] (may be NULL): the candidate that last set the runner-up distance in the reference's update
 * idiom -- what SearchByProjection(Frame&, vector<MapPoint*>&) keeps as bestLevel2 (src/ORBmatcher.cc:128-147): the
 * previous best when a new best arrives, else the first candidate below the runner-up; -1 if fewer than two */
orbfe_status orbfe_hamming_csr_ex(orbfe_matcher *m, const uint8_t *q, int32_t nq, const uint8_t *t, int32_t nt,
                                  const uint32_t *off, const uint32_t *cand, int32_t *best_idx, int32_t *best,
                                  int32_t *second, int32_t *second_idx);
/* every distance of every list: dist[off[nq]] (0..256), for the one caller whose rule needs them all --
 * ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:523-651) skips a candidate that an EARLIER query holds at a
 * distance <= its own (:573), so its best / second-best depend on the matches made so far; the distances come from the
 * device, the in-order rule stays with the caller.  HOST buffers. */
orbfe_status orbfe_hamming_csr_all(orbfe_matcher *m, const uint8_t *q, int32_t nq, const uint8_t *t, int32_t nt,
                                   const uint32_t *off, const uint32_t *cand, uint16_t *dist);
/* DEVICE buffers (queries / train rows e.g. straight out of an extractor output block), enqueued on `stream`, no
 * validation of the candidate indices (they must be < the number of train rows); d_second_idx may be NULL */
orbfe_status orbfe_hamming_csr_device(orbfe_matcher *m, const uint8_t *d_q, int32_t nq, const uint8_t *d_t,
                                      const uint32_t *d_off, const uint32_t *d_cand, int32_t *d_best_idx, int32_t *d_best,
                                      int32_t *d_second, int32_t *d_second_idx, void *stream);

/* the frame grid index that every projection-gated matcher walks.
 * Frame::AssignFeaturesToGrid (src/Frame.cc:319-334) + Frame::PosInGrid (:522-531): 64 x 48 cells over the undistorted
 * image bounds; keypoint i goes to cell (round((x-minx)*gw_inv), round((y-miny)*gh_inv)) if that is inside the grid.
 *   xy[n*2]            undistorted keypoint positions (mvKeysUn[i].pt)
 *   cell_off[64*48+1]  CSR offsets, cell c = ix*48 + iy (= mGrid[ix][iy]);  cell_idx[n]: keypoint indices, ascending per
 *                      cell (push_back order);  *n_in_grid = number of keypoints inside the grid.  HOST buffers. */
#define ORBFE_GRID_COLS 64 /* FRAME_GRID_COLS include/Frame.h:26 */
#define ORBFE_GRID_ROWS 48 /* FRAME_GRID_ROWS include/Frame.h:25 */
orbfe_status orbfe_assign_grid(orbfe_matcher *m, const float *xy, int32_t n, float minx, float miny, float gw_inv,
                               float gh_inv, uint32_t *cell_off, uint32_t *cell_idx, int32_t *n_in_grid);
/* The same index on the host, without a device or a matcher handle: for hosts that hold the keypoints but not the grid
 * (KeyFrame::mGrid is protected in the reference, include/KeyFrame.h:223 -- the matcher shim rebuilds it from the public
 * mvKeysUn with the values Frame::AssignFeaturesToGrid used: Frame::mnMinX / mnMinY, mfGridElement{Width,Height}Inv). */
orbfe_status orbfe_assign_grid_host(const float *xy, int32_t n, float minx, float miny, float gw_inv, float gh_inv,
                                    uint32_t *cell_off, uint32_t *cell_idx, int32_t *n_in_grid);
/* AssignFeaturesToGrid for every frame of an extractor output block, device-resident: frame f's keypoints are
 * d_kps[f * cap .. f * cap + d_n[f]) -- mvKeysUn, so for a camera with lens distortion pass the undistorted block of
 * orbfe_frame_geometry_batch_device, and without distortion (k1 = 0, as for TUM fr3) the block orbfe_extract_batch_device
 * wrote; d_cell_off [nframes][ORBFE_GRID_COLS * ORBFE_GRID_ROWS + 1], d_cell_idx [nframes][cap], d_n_in_grid
 * [nframes].  Enqueued on `stream`, no host synchronisation. */
orbfe_status orbfe_assign_grid_batch_device(orbfe_matcher *m, const orbfe_keypoint *d_kps, const int32_t *d_n, int32_t cap,
                                            int32_t nframes, float minx, float miny, float gw_inv, float gh_inv,
                                            uint32_t *d_cell_off, uint32_t *d_cell_idx, int32_t *d_n_in_grid, void *stream);

/* Frame::GetFeaturesInArea (src/Frame.cc:465-518) for a batch of nq queries (x, y, r, minLevel, maxLevel):
 *   qxyr[nq*3], qlevels[nq*2] (may be NULL = -1,-1);  octave[n] = mvKeysUn[i].octave
 *   off[nq+1], cand[cap]: per query the keypoint indices in the reference's iteration order (ix, iy, cell order).
 * Returns ORBFE_ERR_CAP (with off[nq] = required total) when cap is too small.  Feed (off, cand) to orbfe_hamming_csr
 * to get SearchByProjection's best / second-best per query.  HOST buffers. */
orbfe_status orbfe_features_in_area(orbfe_matcher *m, const float *xy, const int32_t *octave, int32_t n,
                                    const uint32_t *cell_off, const uint32_t *cell_idx, float minx, float miny,
                                    float gw_inv, float gh_inv, const float *qxyr, const int32_t *qlevels, int32_t nq,
                                    uint32_t *off, uint32_t *cand, int32_t cap);

/* GetFeaturesInArea on device buffers, for ONE frame of an extractor output block: d_kps = that frame's keypoint records
 * (x, y, octave are read in place), d_cell_off / d_cell_idx = its grid (orbfe_assign_grid_batch_device), d_qxyr[nq*3] /
 * d_qlevels[nq*2] (may be NULL) the queries; d_off[nq+1] and d_cand[cap] come out in the order orbfe_hamming_csr_device
 * consumes.  Enqueued on `stream`, nothing validated.  If the total exceeds cap nothing is written to d_cand and
 * d_off[nq] (the required size) tells so. */
orbfe_status orbfe_features_in_area_device(orbfe_matcher *m, const orbfe_keypoint *d_kps, const uint32_t *d_cell_off,
                                           const uint32_t *d_cell_idx, float minx, float miny, float gw_inv, float gh_inv,
                                           const float *d_qxyr, const int32_t *d_qlevels, int32_t nq, uint32_t *d_off,
                                           uint32_t *d_cand, int32_t cap, void *stream);

/* the projection-gated searches of the per-frame tracker --
 *   ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th)       src/ORBmatcher.cc:63-157
 *   ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono)   src/ORBmatcher.cc:1578-1724
 *   (and the perfect/ overload that also returns the 2-D point pairs, perfect/src/ORBmatcher.cc:1727-1911).
 * In these HOST-buffer forms the pose projection and its gates (isBad, mbTrackInView, depth sign, image bounds, forward /
 * backward level window) are the caller's (shim/ORBmatcher_orbfe.cc does them on cv::Mat exactly as the reference); the
 * device-resident forms below ("Tracker") run them on the device.  One query = one MapPoint that passed them.  Per query: Frame::GetFeaturesInArea(u, v, r, min_level, max_level) on the frame's grid, the right-image gate
 * (candidate idx skipped when uRight[idx] > 0 && fabs(ur - uRight[idx]) > r -- both call sites compare against the very
 * expression they pass as the search radius, :114-119 / :1654-1660), best / second-best Hamming with the :128-140 idiom
 * over the candidates whose slot is free, acceptance: best <= th (th <= 255; TH_HIGH / ORBdist in the reference) and, with ratio_rule != 0, not (bestLevel == bestLevel2 &&
 * best > nnratio * second) (:143-146; ratio_rule 0 for the last-frame form, :1673).
 * Queries are NOT independent in the reference: an accepted query puts its MapPoint into F.mvpMapPoints[bestIdx], and a
 * slot holding a MapPoint with Observations() > 0 is skipped by every later candidate scan (:108-110 / :1647-1649).
 * blocked[nF] marks slots taken before the call; ORBFE_PROJ_CLAIMS marks a query whose MapPoint has Observations() > 0.
 * The result equals the reference's sequential loop (fixed point by relaxation).
 *   match[nq]: frame feature assigned to query i, -1 = none.  The caller replays, in query order,
 *              F.mvpMapPoints[match[i]] = pMP_i; nmatches++  (later queries may overwrite a slot whose point has no
 *              observations: the reference counts both), then its rotation histogram (:1683-1721) where it has one.
 *   best / second[nq] (may be NULL): bestDist / bestDist2 of the scan that decided the query (256 = none).
 * HOST buffers; xyF = mvKeysUn[i].pt, octF = mvKeysUn[i].octave, (cell_off, cell_idx) = Frame::mGrid as orbfe_assign_grid
 * lays it out; at most 15360 frame features. */
typedef struct orbfe_proj_query {
    float u, v, r;                   /* GetFeaturesInArea(u, v, r, min_level, max_level) */
    int32_t min_level, max_level;
    float ur;                        /* projected right-image coordinate (mTrackProjXR / u - mbf * invzc) */
    int32_t flags;                   /* ORBFE_PROJ_* */
    int32_t pad;
} orbfe_proj_query;
#define ORBFE_PROJ_CLAIMS 1          /* the query's MapPoint has Observations() > 0: its slot is skipped by later queries */
#define ORBFE_PROJ_RIGHT_GATE 2      /* apply the right-image gate (both Frame overloads do; the KeyFrame forms do not) */
#define ORBFE_PROJ_CHI2_GATE 4       /* Fuse (src/ORBmatcher.cc:1112-1139): skip a candidate whose reprojection error
                                      * e2 * inv_level_sigma2[octave] exceeds 7.8 (uRight[idx] >= 0: e2 = ex^2 + ey^2 + er^2,
                                      * er = ur - uRight[idx]) / 5.99 (monocular keypoint); needs the _chi2 entry point */
orbfe_status orbfe_search_by_projection(orbfe_matcher *m, const uint8_t *descF, const float *xyF, const int32_t *octF,
                                        int32_t nF, const uint32_t *cell_off, const uint32_t *cell_idx, float minx, float miny,
                                        float gw_inv, float gh_inv, const float *uRight /* nF or NULL */,
                                        const uint8_t *blocked /* nF or NULL */, const orbfe_proj_query *q,
                                        const uint8_t *qdesc /* nq x 32 */, int32_t nq, int32_t th, float nnratio,
                                        int32_t ratio_rule, int32_t *match, int32_t *best, int32_t *second);

/* the same search with the per-level table the ORBFE_PROJ_CHI2_GATE queries need (KeyFrame::mvInvLevelSigma2); the other
 * members of the family use it without claims: ORBmatcher::Fuse x2 (src/ORBmatcher.cc:1031, :1198) and SearchBySim3 (:1334)
 * pass flags without ORBFE_PROJ_CLAIMS, blocked = NULL, ratio_rule 0 and read match[i] = the best candidate if its distance is
 * <= th, so that GetFeaturesInArea runs on the device for them too */
orbfe_status orbfe_search_by_projection_chi2(orbfe_matcher *m, const uint8_t *descF, const float *xyF, const int32_t *octF,
                                             int32_t nF, const uint32_t *cell_off, const uint32_t *cell_idx, float minx, float miny,
                                             float gw_inv, float gh_inv, const float *uRight /* nF or NULL */,
                                             const uint8_t *blocked /* nF or NULL */, const float *inv_level_sigma2 /* nlevels or NULL */,
                                             int32_t nlevels, const orbfe_proj_query *q, const uint8_t *qdesc /* nq x 32 */, int32_t nq,
                                             int32_t th, float nnratio, int32_t ratio_rule, int32_t *match, int32_t *best,
                                             int32_t *second);

/* HOST-side geometry of the same family (csrc/orbfe_hostgeom.hip; no device, no handle), so that a host shim only flattens
 * its objects and replays decisions.  Arithmetic order = what the reference's cv::Mat expressions evaluate to: 3x3 * 3x1
 * products accumulate left to right in float, norms and dot products in double, nothing fused.
 *
 * orbfe_project_points: x_c = R * x_w + t (then x_c = R2 * x_c + t2 when R2 != NULL: SearchBySim3's two stages), the depth /
 * image / distance / viewing-angle gates and the projected coordinates of n map points -- src/ORBmatcher.cc:401-433 (Sim3
 * projection), :1060-1101 (Fuse), :1224-1255 (Fuse, Sim3), :1389-1424 (SearchBySim3), :1620-1642 (last frame), :1778-1803
 * (relocalisation).  ok[i] = 1 when point i passed every gate; u, v (and invz, dist, ur = u - bf * invz where non-NULL) are
 * written for those.  min_dist / max_dist NULL: no distance gate; with them dist = |x_w - Ow| (Ow != NULL) or |x_c|; normal
 * != NULL adds the viewing-angle gate PO . n < 0.5 * dist -> out.  R, R2 row-major 3x3. */
#define ORBFE_PJ_SKIP_NEG_DEPTH 1    /* z_c < 0 -> out (:411, :1068, :1234, :1396) */
#define ORBFE_PJ_SKIP_NEG_INVZ 2     /* 1 / z_c < 0 -> out (:1625) */
#define ORBFE_PJ_UV_CHAINED 4        /* u = fx * x_c * invz + cx (:1627, :1789) instead of u = fx * (x_c * invz) + cx */
#define ORBFE_PJ_BOUNDS_CLOSED 8     /* out iff u < minx || u > maxx (Frame statics, :1629) instead of KeyFrame::IsInImage */
orbfe_status orbfe_project_points(const float *R, const float *t, const float *R2, const float *t2, const float *Ow, float fx,
                                  float fy, float cx, float cy, float bf, float minx, float maxx, float miny, float maxy,
                                  int32_t flags, int32_t n, const float *world_pos, const float *normal, const float *min_dist,
                                  const float *max_dist, float *u, float *v, float *invz, float *dist, float *ur, uint8_t *ok);
/* the gating of SearchByProjection(Frame&, const vector<MapPoint*>&, th) (:63-93; Tracking::SearchLocalPoints): points with
 * mbTrackInView and !isBad() become queries (u, v, ur) = proj_uvr[i], r = RadiusByViewingCos(view_cos) [* th] *
 * scale_factors[level], levels [level - 1, level], right-image gate on, CLAIMS iff obs_gt0; q / src compacted, *nq their count */
orbfe_status orbfe_proj_queries_local_map(const float *scale_factors, int32_t n, const uint8_t *in_view, const uint8_t *bad,
                                          const int32_t *level, const float *view_cos, const float *proj_uvr, const uint8_t *obs_gt0,
                                          float th, orbfe_proj_query *q, int32_t *src, int32_t *nq);
/* the rotation-consistency check every matcher ends with: match i votes for bin round((angle_a[i] - angle_b[i], + 360 if
 * negative) * (1 / histo_len)) (:308-313), the three fullest bins stay (ComputeThreeMaxima :1912-1957: an earlier bin wins a
 * tie, the second / third go when under a tenth of the first); drop[i] = 1 for matches outside them.  A match whose bin is
 * not in [0, histo_len] (NaN, an angle outside [0, 360), or histo_len < 19 with ordinary angles) is what the reference asserts
 * against (:314): ORBFE_ERR_ARG, nothing written */
orbfe_status orbfe_rotation_consistency(const float *angle_a, const float *angle_b, int32_t n, int32_t histo_len, uint8_t *drop);
/* SearchForInitialization's in-order rule (:547-617) on the lists of orbfe_window_distances: query qi takes its closest
 * candidate among those no earlier query holds at a distance <= its own, accepted when best <= th and best < second * nnratio;
 * a later query may take a held feature over.  accepted[nq]: the feature a query was accepted with (-1: none) -- whether or
 * not it was taken over later; holder[n2]: the query that holds a feature at the end (-1: none). */
orbfe_status orbfe_initialization_resolve(const uint32_t *off, const uint32_t *ent, int32_t nq, int32_t n2, int32_t th, float nnratio,
                                          int32_t *accepted, int32_t *holder);

/* The window search and the distances alone, as lists: off[nq + 1], ent[off[nq]] with ent = feature | distance << 16 in the
 * reference's candidate order (GetFeaturesInArea's cell walk); flags / ur of the queries are ignored.  ORBFE_ERR_CAP (off[nq] =
 * the size needed) when cap is too small.  ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:523-651) runs its in-order
 * rule -- a candidate held by an earlier query at a smaller distance is skipped, :571-574 -- on these lists.  HOST buffers. */
orbfe_status orbfe_window_distances(orbfe_matcher *m, const uint8_t *descF, const float *xyF, const int32_t *octF, int32_t nF,
                                    const uint32_t *cell_off, const uint32_t *cell_idx, float minx, float miny, float gw_inv,
                                    float gh_inv, const orbfe_proj_query *q, const uint8_t *qdesc, int32_t nq, uint32_t *off,
                                    uint32_t *ent, int32_t cap);

/* the matching core of ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:827-1012,
 * LocalMapping::CreateNewMapPoints).  For every feature of keyframe 1 with elig1 (no MapPoint; stereo if bOnlyStereo) whose
 * vocabulary node also exists in keyframe 2: over that node's keyframe-2 features in FeatureVector order, the ones with elig2
 * (no MapPoint; stereo if bOnlyStereo -- the reference's loop never sets vbMatched2, so the keyframe-1 features are
 * independent), dist <= th_low, dist <= bestDist, farther than the epipole gate ((ex - x)^2 + (ey - y)^2 >= 100 * scale[octave],
 * applied only when both keypoints are monocular, :900-907) and inside CheckDistEpipolarLine (:175-196: F12 row-major,
 * dsqr < 3.84 * mvLevelSigma2[octave], the reference's float operation order) take over the best: the smallest distance, the
 * LAST in order on ties.  match12[n1] = keyframe-2 feature or -1; the caller applies its rotation histogram (:966-985) and
 * builds vMatchedPairs.  FeatureVectors as CSR (ascending node ids); HOST buffers. */
orbfe_status orbfe_search_for_triangulation(orbfe_matcher *m, const uint8_t *desc1, const float *xy1, const uint8_t *elig1,
                                            const uint8_t *stereo1, int32_t n1, const uint32_t *node1, const uint32_t *off1,
                                            const uint32_t *idx1, int32_t nn1, const uint8_t *desc2, const float *xy2,
                                            const int32_t *oct2, const uint8_t *elig2, const uint8_t *stereo2, int32_t n2,
                                            const uint32_t *node2, const uint32_t *off2, const uint32_t *idx2, int32_t nn2,
                                            const float F12[9], float ex, float ey, const float *scale_factors2,
                                            const float *level_sigma2_2, int32_t nlevels2, int32_t th_low, int32_t *match12);

/* Tracker: the two projection searches Tracking runs on every frame -- SearchByProjection(CurrentFrame, LastFrame, th, bMono)
 * (TrackWithMotionModel, the fork's TrackHomo) and SearchByProjection(F, vpMapPoints, th) (SearchLocalPoints) -- batched and
 * device-resident, with the pose projection and its gates ON THE DEVICE (csrc/orbfe_track.hip; the per-point arithmetic is
 * csrc/orbfe_track_geom.h, host and device alike).  Every call is enqueued on `stream`, none waits for the device, none
 * writes host memory; scratch is the matcher's.  Batch layout = the other *_batch_device calls: frame f's keypoints are
 * d_kps[f * cap .. f * cap + d_n[f]), descriptors d_desc[(f * cap + i) * 32], the grid of orbfe_assign_grid_batch_device, depth /
 * uRight of orbfe_frame_geometry_batch_device, poses d_Tcw[f][12] = row-major 3x4 (Rcw | tcw).  Limits: cap <= 15360,
 * th <= 255, nlevels <= 16, nframes * qcap < 2^25.  DESIGN.md 8k. */
typedef struct orbfe_track_camera {
    float fx, fy, cx, cy, bf;
    float minx, maxx, miny, maxy;    /* Frame::mnMinX .. mnMaxY (orbfe_image_bounds) */
} orbfe_track_camera;
/* the frames that are searched ("current" frames) */
typedef struct orbfe_track_frames {
    const orbfe_keypoint *d_kps;     /* [nframes][cap], mvKeysUn */
    const uint8_t *d_desc;           /* [nframes][cap][32] */
    const int32_t *d_n;              /* [nframes] */
    int32_t cap;
    const uint32_t *d_cell_off;      /* [nframes][ORBFE_GRID_COLS * ORBFE_GRID_ROWS + 1] */
    const uint32_t *d_cell_idx;      /* [nframes][cap] */
    float minx, miny, gw_inv, gh_inv;
    const float *d_uright;           /* [nframes][cap] or NULL (no right-image gate) */
    const uint8_t *d_slot;           /* [nframes][cap] or NULL: mvpMapPoints[i] before the call -- 0 NULL, 1 a MapPoint with
                                      * Observations() == 0, 2 one with Observations() > 0 (candidate scans skip the slot) */
} orbfe_track_frames;
/* the "last" frames of the last-frame form: a separate pointer set, so a sequence passes its own block shifted by one frame
 * and a replay pairs arbitrary frames */
typedef struct orbfe_track_last {
    const orbfe_keypoint *d_kps;     /* [nframes][cap]: octave and angle are read */
    const int32_t *d_n;              /* [nframes] */
    int32_t cap;
    const uint8_t *d_valid;          /* [nframes][cap]: has a MapPoint && !mvbOutlier */
    const float *d_world_pos;        /* [nframes][cap][3] */
    const uint8_t *d_obs_gt0;        /* [nframes][cap]: Observations() > 0 */
    const uint8_t *d_mpdesc;         /* [nframes][cap][32]: MapPoint::GetDescriptor() (a created point: the keypoint's own row) */
    const float *d_Tcw;              /* [nframes][12] */
} orbfe_track_last;
/* the map as flat point arrays */
typedef struct orbfe_track_map {
    const float *d_world_pos, *d_normal;       /* [npoints][3] */
    const float *d_min_dist, *d_max_dist;      /* GetMinDistanceInvariance / GetMaxDistanceInvariance */
    const uint8_t *d_bad, *d_obs_gt0;
    const uint8_t *d_desc;                     /* [npoints][32]; read by the search only */
    int32_t npoints;
} orbfe_track_map;
/* what isInFrustum leaves in a MapPoint: mTrackProjX / Y / XR, mTrackViewCos, mnTrackScaleLevel (level -1: not in view) */
typedef struct orbfe_track_proj {
    float u, v, ur, view_cos;
    int32_t level;
} orbfe_track_proj;
/* results of a chain call; d_pairs / d_npairs may be NULL */
typedef struct orbfe_track_out {
    orbfe_proj_query *d_q;           /* [nframes][qcap] the queries, compacted in source order */
    int32_t *d_qsrc;                 /* [nframes][qcap] last-frame feature / map point of each query */
    int32_t *d_nq;                   /* [nframes] */
    int32_t qcap;
    int32_t *d_match, *d_best, *d_second;   /* [nframes][qcap] as orbfe_search_by_projection */
    int32_t *d_status;               /* [2]: entries needed when ent_cap was too small (else 0); most rounds any frame ran */
    int32_t *d_assigned;             /* [nframes][cap]: -1 NULL, -2 the MapPoint the slot held before, else the source that took it */
    int32_t *d_nmatches;             /* [nframes] the reference's return value */
    int32_t *d_pairs, *d_npairs;     /* [nframes][qcap][2] (source, current feature) in match order; [nframes] their count */
} orbfe_track_out;

/* Frame::UnprojectStereo (src/Frame.cc:879-899) of every keypoint with d_depth > 0 into d_world_pos [nframes][cap][3] (zeros
 * elsewhere), and the selection of Tracking::UpdateLastFrame (:1833-1883): sorted by (depth, index), all points up to
 * th_depth, at least 100, one more than either.  d_keeps [nframes][cap] (may be NULL): the slot holds a MapPoint with
 * Observations() >= 1; d_created = selected && !keeps.  Localisation-only mode and the mnLastKeyFrameId early return are the
 * caller's `if`. */
orbfe_status orbfe_unproject_select_batch_device(orbfe_matcher *m, const orbfe_keypoint *d_kps, const float *d_depth, const int32_t *d_n,
                                                 int32_t cap, int32_t nframes, const float *d_Tcw, const orbfe_track_camera *cam,
                                                 float th_depth, const uint8_t *d_keeps, float *d_world_pos, uint8_t *d_created,
                                                 void *stream);
/* the gating of the last-frame form (src/ORBmatcher.cc:1590-1644, operation order of the oracle's orc_proj_queries_last_frame):
 * projection, invzc < 0, closed image bounds, forward / backward level window from tlc against mb (unless mono), r = th *
 * scale_factors[octave], ur = u - bf * invzc, RIGHT_GATE | CLAIMS iff obs_gt0.  A keypoint whose octave is outside
 * [0, nlevels) makes no query.  Queries are compacted in feature order (no atomics take a slot); those past qcap are dropped,
 * d_nq[f] <= qcap.  scale_factors is a HOST array. */
orbfe_status orbfe_gate_last_frame_batch_device(orbfe_matcher *m, const float *d_Tcw_cur, const orbfe_track_last *last,
                                                const orbfe_track_camera *cam, float mb, int32_t mono, float th, const float *scale_factors,
                                                int32_t nlevels, int32_t nframes, orbfe_proj_query *d_q, int32_t *d_qsrc, int32_t *d_nq,
                                                int32_t qcap, void *stream);
/* Frame::isInFrustum(pMP, 0.5) (src/Frame.cc:387-451) with MapPoint::PredictScale (src/MapPoint.cc:465-480) and the gating of
 * SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:63-93) for every frame's list of local map points: frame f's list
 * is d_list_idx[d_list_off[f] .. d_list_off[f + 1]) (indices into `map`), d_seen[entry] (may be NULL) = mnLastFrameSeen ==
 * mnId.  d_qsrc holds map point indices; d_visible[f] (may be NULL) = nToMatch; d_proj[nentries] (may be NULL) what
 * isInFrustum left in each entry's MapPoint.  An entry whose index is outside [0, map->npoints) makes no query and leaves
 * level -1 and zeros in d_proj, like an entry that is seen, bad or out of view.  Offsets beyond nentries are cut there (a
 * list that starts beyond it is empty); queries past qcap are dropped, d_nq[f] <= qcap, while d_visible[f] keeps the full
 * count.  PcZ == 0 is undefined here as in the reference (NaN passes its bounds test). */
orbfe_status orbfe_gate_local_map_batch_device(orbfe_matcher *m, const float *d_Tcw, const orbfe_track_camera *cam, float th,
                                               const float *scale_factors, int32_t nlevels, float log_scale_factor,
                                               const orbfe_track_map *map, const uint32_t *d_list_off, const int32_t *d_list_idx,
                                               const uint8_t *d_seen, int64_t nentries, int32_t nframes, orbfe_proj_query *d_q,
                                               int32_t *d_qsrc, int32_t *d_nq, int32_t qcap, int32_t *d_visible, orbfe_track_proj *d_proj,
                                               void *stream);
/* the same arithmetic on the HOST for n points of one frame (no device, no handle): proj[n], in_view[n]; seen / bad may be NULL */
orbfe_status orbfe_frustum_points(const float *Tcw, const orbfe_track_camera *cam, float log_scale_factor, int32_t nlevels, int32_t n,
                                  const float *world_pos, const float *normal, const float *min_dist, const float *max_dist,
                                  const uint8_t *seen, const uint8_t *bad, orbfe_track_proj *proj, uint8_t *in_view);
/* orbfe_search_by_projection for a batch: query i of frame f is d_q[f * qcap + i], i < d_nq[f] (read on the device), its
 * descriptor row d_qsrc[f * qcap + i] of the pool d_qpool + f * pool_frame_rows * 32 (pool_frame_rows 0: one pool for all
 * frames; a row outside [0, pool_rows) finds nothing).  Candidate entries of all frames go into ONE buffer of ent_cap entries
 * in the matcher's scratch; when it is too small nothing is written past any buffer, d_match is -1 everywhere and
 * d_status[0] holds the exact need -- call again with it.  inv_level_sigma2 (HOST, may be NULL) as in the _chi2 form. */
orbfe_status orbfe_search_by_projection_batch_device(orbfe_matcher *m, const orbfe_track_frames *frames, int32_t nframes,
                                                     const orbfe_proj_query *d_q, const int32_t *d_qsrc, const int32_t *d_nq, int32_t qcap,
                                                     const uint8_t *d_qpool, int32_t pool_rows, int32_t pool_frame_rows,
                                                     const float *inv_level_sigma2, int32_t nlevels, int32_t th, float nnratio,
                                                     int32_t ratio_rule, int64_t ent_cap, int32_t *d_match, int32_t *d_best,
                                                     int32_t *d_second, int32_t *d_status, void *stream);
/* what the reference's loop leaves behind, from the core's matches: d_assigned starts from frames->d_slot, a slot takes the
 * LAST query in order that matched it; with check_ori the 30-bin rotation histogram (angle of d_last_kps[f][source] minus
 * the current keypoint's) and ComputeThreeMaxima: a slot goes back to -1 if ANY match to it lies in a dropped bin, d_nmatches
 * = matches - dropped entries (a slot matched twice counts twice, as in the reference). */
orbfe_status orbfe_track_replay_batch_device(orbfe_matcher *m, const orbfe_track_frames *frames, int32_t nframes, const int32_t *d_match,
                                             const int32_t *d_qsrc, const int32_t *d_nq, int32_t qcap, const orbfe_keypoint *d_last_kps,
                                             int32_t cap_last, int32_t check_ori, int32_t *d_assigned, int32_t *d_nmatches,
                                             int32_t *d_pairs, int32_t *d_npairs, void *stream);
/* gating -> search -> replay in one call.  Last frame: ratio rule off (:1673), th_high = TH_HIGH; d_pairs feed
 * orbfe_find_homographies_device as the perfect/ overload's points_last / points_current.  Local map: ratio rule on. */
orbfe_status orbfe_track_last_frame_batch_device(orbfe_matcher *m, const orbfe_track_frames *cur, const float *d_Tcw_cur,
                                                 const orbfe_track_last *last, const orbfe_track_camera *cam, float mb, int32_t mono,
                                                 float th, const float *scale_factors, int32_t nlevels, int32_t th_high, int32_t check_ori,
                                                 int64_t ent_cap, int32_t nframes, const orbfe_track_out *out, void *stream);
orbfe_status orbfe_track_local_map_batch_device(orbfe_matcher *m, const orbfe_track_frames *cur, const float *d_Tcw,
                                                const orbfe_track_camera *cam, float th, const float *scale_factors, int32_t nlevels,
                                                float log_scale_factor, const orbfe_track_map *map, const uint32_t *d_list_off,
                                                const int32_t *d_list_idx, const uint8_t *d_seen, int64_t nentries, int32_t th_high,
                                                float nnratio, int64_t ent_cap, int32_t nframes, const orbfe_track_out *out,
                                                int32_t *d_visible, orbfe_track_proj *d_proj, void *stream);
/* bytes of matcher scratch the search takes for (nframes, qcap, ent_cap); -1 outside the limits.  No device needed. */
int64_t orbfe_track_scratch_bytes(int32_t nframes, int32_t qcap, int64_t ent_cap);

/* SearchForInitialization: ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:523-651, Tracking::MonocularInitialization) for
 * a batch of frame pairs, device-resident (csrc/orbfe_init_search.hip), so that extractor -> grid -> this call ->
 * orbfe_initializer_initialize_device runs on one stream without a host read.  Bit for bit the reference's loop:
 *   For every feature i1 of frame 1 with octave == 0, in index order:
 *   1. GetFeaturesInArea(prev[i1].x, prev[i1].y, window, 0, 0) on frame 2's grid gives the candidates, in the cell-walk order.
 *   2. A candidate i2 at Hamming distance d is SKIPPED when held[i2] <= d; held[i2] is the distance at which an earlier query
 *      was accepted on i2 (INT_MAX if none).  Every acceptance lowers it, so it is the minimum over the accepted earlier queries.
 *   3. Over the rest, best and second-best by the `dist < bestDist ... else if dist < bestDist2` idiom: the first in list order
 *      wins a tie.
 *   4. Accepted when bestDist <= th_low and (float)bestDist < (float)bestDist2 * nnratio (one float multiply; bestDist2 = INT_MAX
 *      without a second candidate).
 *   5. Acceptance takes the feature over: the previous holder's matches12 entry goes back to -1 (nmatches - 1), the new query
 *      holds it (nmatches + 1).
 *   6. With check_ori every ACCEPTED query votes in the 30-bin rotation histogram (angle of frame 1's keypoint minus frame 2's,
 *      times 1/30, rounded, 30 -> 0), whether or not it is taken over later.
 *   7. After ComputeThreeMaxima a vote in a dropped bin clears matches12[i1] and decrements nmatches only if that entry still
 *      stands.
 *   8. prev[i1] = keys2[matches12[i1]].pt for the matches that stand; every other prev entry keeps its value.
 * The sequential result is the unique fixed point of "every query decides against the claims of the earlier queries"; the device
 * reaches it by rounds over per-feature claim lists (a single word per feature -- the smallest distance, or the lowest query --
 * decides some legal inputs wrongly: DESIGN.md 8l).
 * Batch layout = the Tracker's: pair p's first frame is first->d_kps[p * cap .. p * cap + d_n[p]) with descriptors d_desc[(p * cap
 * + i) * 32], its second frame `second` (grid of orbfe_assign_grid_batch_device; d_uright and d_slot are not read).  Counts are
 * clamped into [0, cap].  d_prev_in [npairs][cap1][2] is vbPrevMatched; NULL = the features' own positions (Tracking :622-624).
 * Limits: cap <= 15360 in both frames, th_low <= 255, npairs * first->cap < 2^25. */
typedef struct orbfe_init_search_first {
    const orbfe_keypoint *d_kps;     /* [npairs][cap], mvKeysUn: x, y, angle, octave are read */
    const uint8_t *d_desc;           /* [npairs][cap][32] */
    const int32_t *d_n;              /* [npairs] */
    int32_t cap;                     /* cap1 >= 1 */
} orbfe_init_search_first;
typedef struct orbfe_init_search_out {
    int32_t *d_matches12;            /* [npairs][cap1]: vnMatches12; -1 for features that are not level-0, unmatched, taken over,
                                      * dropped, or >= n1 */
    int32_t *d_nmatches;             /* [npairs] the reference's return value */
    float *d_prev_out;               /* [npairs][cap1][2] or NULL: vbPrevMatched after the call; may equal d_prev_in */
    /* The pairs packed by their counts, as orbfe_initializer_initialize_device takes them (its Normalize runs over ALL keys of
     * a frame, so rows padded to cap would change T1 / T2).  Each may be NULL; the packed arrays need their offsets.  Room for
     * npairs * cap entries; what lies past d_offsets[npairs] keeps what it held. */
    int32_t *d_offsets1, *d_offsets2; /* [npairs + 1]: prefix sums of the clamped counts of the first / second frames */
    int32_t *d_matches12_csr;        /* pair p's d_matches12 row [0, n1) from d_offsets1[p] on */
    float *d_keys1_xy;               /* [.][2] mvKeysUn[i].pt of the first frames, by d_offsets1 ... */
    float *d_keys2_xy;               /* [.][2] ... and of the second frames, by d_offsets2 */
    int32_t *d_status;               /* [2]: entries needed when ent_cap was too small (else 0); most rounds any pair ran */
} orbfe_init_search_out;
/* Enqueued on `stream`: no wait, no host writes; scratch is the matcher's.  min_matches: 0 = off (Tracking uses 100); a pair
 * with nmatches < min_matches gets its d_matches12 row (and its part of d_matches12_csr) all -1, so that the Initializer reports ORBFE_INIT_FEW_MATCHES for it,
 * while d_nmatches and d_prev_out keep the reference's values.  When the candidate entries of all pairs exceed ent_cap every
 * row is -1, d_nmatches is 0, d_prev_out is a copy of the input and d_status[0] holds the exact need: call again with it. */
orbfe_status orbfe_search_for_initialization_batch_device(orbfe_matcher *m, const orbfe_init_search_first *first,
                                                          const orbfe_track_frames *second, int32_t npairs, const float *d_prev_in,
                                                          int32_t window, int32_t th_low, float nnratio, int32_t check_ori,
                                                          int32_t min_matches, int64_t ent_cap, const orbfe_init_search_out *out,
                                                          void *stream);
/* One pair on HOST arrays, synchronous on the matcher's stream: upload, the same launches, download (the entry buffer is grown
 * and the call repeated inside when it was short).  xy = mvKeysUn[i].pt, octave, angle, descriptors of both frames, frame 2's
 * grid as orbfe_assign_grid lays it out; prev [n1][2] is vbPrevMatched, read and written; matches12 [n1]; *nmatches = the
 * reference's return value. */
orbfe_status orbfe_search_for_initialization(orbfe_matcher *m, const float *xy1, const int32_t *oct1, const float *ang1,
                                             const uint8_t *desc1, int32_t n1, const float *xy2, const int32_t *oct2, const float *ang2,
                                             const uint8_t *desc2, int32_t n2, const uint32_t *cell_off, const uint32_t *cell_idx,
                                             float minx, float miny, float gw_inv, float gh_inv, float *prev, int32_t window,
                                             int32_t th_low, float nnratio, int32_t check_ori, int32_t *matches12, int32_t *nmatches);
/* bytes of matcher scratch the batch form takes for (npairs, cap1, ent_cap); -1 outside the limits.  No device needed. */
int64_t orbfe_init_search_scratch_bytes(int32_t npairs, int32_t cap1, int64_t ent_cap);

/* SearchForTriangulation, batched: ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:827-1019) for the neighbour loop of
 * LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:349-422) -- one keyframe against all its covisible neighbours, or many
 * keyframes of a replayed sequence against theirs -- device-resident (csrc/orbfe_tri_search.hip), so that extractor ->
 * orbfe_frame_geometry_batch_device -> orbfe_bow_transform_batch_device -> orbfe_triangulation_pairs_batch_device -> this call run
 * on one stream without a host read.  It stops at vMatchedPairs and takes d_has_mp as a constant: the triangulation of the pairs
 * (:424-610), KeyFrame::ComputeSceneMedianDepth (the d_median_depth input of the monocular baseline gate) and the loop that carries
 * the filled slots from neighbour to neighbour are "CreateNewMapPoints, device-resident" below.
 *
 * The keyframe block, batch layout of the other *_batch_device calls: keyframe b owns `cap` slots of every array (cap + 1 of
 * d_fv_off, 4 of d_counts); the FeatureVector arrays are exactly what orbfe_bow_transform_batch_device writes.  Pair p matches
 * keyframe d_kf1[p] (the current keyframe, "1") against d_kf2[p]; the same keyframe may be keyframe 1 of many pairs and a pair
 * (i, i) is legal.  Per pair, bit for bit what orbfe_search_for_triangulation + the reference's replay give:
 *   - a feature of either keyframe takes part iff its slot holds no MapPoint (d_has_mp == 0) and, with only_stereo, uRight >= 0;
 *   - every such keyframe-1 feature whose vocabulary node exists in keyframe 2 takes, among that node's keyframe-2 features that
 *     pass dist <= th_low, the epipole gate (both keypoints monocular: (ex - x)^2 + (ey - y)^2 >= 100 * scale[octave]) and
 *     CheckDistEpipolarLine (dsqr < 3.84 * sigma2[octave]; den == 0 fails), the smallest distance, the LAST in list order on ties;
 *   - with check_ori the 30-bin histogram of kp1.angle - kp2.angle (times 1.0f / 30, sic) and ComputeThreeMaxima clear the matches
 *     of the other bins.
 * Counts (d_n, d_counts[1], the offsets) are clamped into [0, cap].  Three things cannot be rejected without reading device
 * memory on the host, and each is simply not a candidate or not a query: a keyframe-2 feature whose octave is outside
 * [0, nlevels), a d_fv_idx entry >= the keyframe's d_n, and a frame index outside [0, nframes) (that pair gets an all -1 row
 * and 0 matches, like a skipped one).
 * Limits: cap <= 8192 (the BoW block's), th_low <= 255, nlevels <= 16, npairs * cap < 2^25. */
typedef struct orbfe_tri_keyframes {
    const orbfe_keypoint *d_kps;     /* [nframes][cap], mvKeysUn: x, y, angle, octave are read */
    const uint8_t *d_desc;           /* [nframes][cap][32] */
    const int32_t *d_n;              /* [nframes] */
    int32_t cap, nframes;
    const float *d_uright;           /* [nframes][cap] mvuRight: stereo means >= 0; NULL = every keypoint is monocular */
    const uint8_t *d_has_mp;         /* [nframes][cap] GetMapPoint(i) != NULL; NULL = no slot holds a MapPoint */
    const uint32_t *d_fv_node, *d_fv_off, *d_fv_idx;   /* [nframes][cap], [nframes][cap + 1], [nframes][cap] */
    const int32_t *d_counts;         /* [nframes][4]: [1] = number of nodes */
} orbfe_tri_keyframes;
typedef struct orbfe_tri_out {
    int32_t *d_match12;              /* [npairs][cap]: keyframe-2 feature of keyframe-1 feature i after the rotation check, -1 none
                                      * (also for i >= n1) */
    int32_t *d_nmatches;             /* [npairs] the reference's return value */
    int32_t *d_pairs;                /* [npairs][cap][2] (idx1, idx2) in ascending idx1 = vMatchedPairs; rows past d_npairs[p] keep
                                      * what they held.  NULL together with d_npairs: not wanted */
    int32_t *d_npairs;               /* [npairs] */
} orbfe_tri_out;
/* Enqueued on `stream`: no wait, no host writes; scratch is the matcher's.  d_F12 [npairs][9] row-major and d_epi [npairs][2]
 * (ex, ey: the epipole of keyframe 1 in keyframe 2) are plain inputs -- orbfe_triangulation_pairs_batch_device makes them;
 * d_pair_skip [npairs] (may be NULL): a pair with a non-zero byte gets an all -1 row and nmatches 0.  scale_factors / level_sigma2
 * are HOST arrays of nlevels floats (mvScaleFactors / mvLevelSigma2 of keyframe 2). */
orbfe_status orbfe_search_for_triangulation_batch_device(orbfe_matcher *m, const orbfe_tri_keyframes *kf, const int32_t *d_kf1,
                                                         const int32_t *d_kf2, int32_t npairs, const float *d_F12, const float *d_epi,
                                                         const uint8_t *d_pair_skip, const float *scale_factors,
                                                         const float *level_sigma2, int32_t nlevels, int32_t th_low,
                                                         int32_t only_stereo, int32_t check_ori, const orbfe_tri_out *out, void *stream);
/* What CreateNewMapPoints computes per neighbour before the search (src/LocalMapping.cc:390-417, src/ORBmatcher.cc:833-843), one
 * thread per pair: d_pair_skip = the baseline gate (|Ow2 - Ow1| accumulated in double, sqrt, stored as float; stereo / RGB-D:
 * skipped iff baseline < mb; mono: iff baseline / d_median_depth[kf2] < 0.01), d_F12 = ComputeF12, d_epi = the epipole.  d_Tcw
 * [nframes][12] row-major 3x4 (Rcw | tcw), d_Ow [nframes][3] = KeyFrame::GetCameraCenter (the caller's); d_median_depth [nframes]
 * = ComputeSceneMedianDepth(2), required when mono; both keyframes share `cam` (fx, fy, cx, cy are read).  A pair with a frame
 * index outside [0, nframes) is skipped, with zeros in d_F12 / d_epi. */
orbfe_status orbfe_triangulation_pairs_batch_device(orbfe_matcher *m, const float *d_Tcw, const float *d_Ow, int32_t nframes,
                                                    const orbfe_track_camera *cam, float mb, int32_t mono, const float *d_median_depth,
                                                    const int32_t *d_kf1, const int32_t *d_kf2, int32_t npairs, float *d_F12,
                                                    float *d_epi, uint8_t *d_pair_skip, void *stream);
/* LocalMapping::ComputeF12 (:848-867) on the HOST, the function the kernel runs (csrc/orbfe_f12.h; no device, no handle):
 * K1.t().inv() * t12x * R12 * K2.inv() with cv::invert's 3x3 case and cv::gemm's small-matrix rules.  Bit-exact against
 * tests/f12_oracle.py, a restatement no compiled reference pins; K1.t().inv() * t12x is taken as invert-then-multiply, where
 * OpenCV's MatExpr runs an LU solve.  Tcw1 / Tcw2 [12], F12 [9] row-major. */
orbfe_status orbfe_compute_f12(const float *Tcw1, const float *Tcw2, const orbfe_track_camera *cam, float *F12);
/* bytes of matcher scratch the batch form takes for (npairs, cap); -1 outside the limits.  No device needed. */
int64_t orbfe_tri_search_scratch_bytes(int32_t npairs, int32_t cap);
/* the constants of the search kernel (tests take their list lengths from here); -1 for an unknown `what`.  No device needed. */
#define ORBFE_TRI_INFO_LANES 0             /* lanes that share one keyframe-1 feature */
#define ORBFE_TRI_INFO_TILE 1              /* keyframe-2 features per LDS tile */
#define ORBFE_TRI_INFO_QUERIES_PER_PASS 2  /* keyframe-1 features a workgroup handles at once */
#define ORBFE_TRI_INFO_NODE_WORKGROUPS 3   /* workgroups per pair; the keyframe-1 nodes are dealt to them round robin */
#define ORBFE_TRI_INFO_MAX_CAP 4
int32_t orbfe_tri_search_info(int32_t what);
/* 0 = k_tri_search (LDS tiles, a group of lanes per feature; default), 1 = one thread per keyframe-1 feature: same results */
orbfe_status orbfe_matcher_set_triangulation_kernel(orbfe_matcher *m, int32_t kernel);

/* CreateNewMapPoints, device-resident: the rest of the neighbour loop of LocalMapping::CreateNewMapPoints up to
 * `new MapPoint(x3D, ...)` (src/LocalMapping.cc:424-615) and KeyFrame::ComputeSceneMedianDepth (src/KeyFrame.cc:724-754), on the
 * keyframe block of the batched search (csrc/orbfe_newpoints.hip, csrc/orbfe_newpoints.h).  The oracle is
 * tests/newpoints_oracle.py, a numpy restatement under numbered rules (N1 ..) that NO compiled reference pins: LocalMapping.cc and
 * KeyFrame.cc are not among the compiled reference sources.
 *
 * The verdict of one match = where the loop body left, in the order the reference can leave it: */
#define ORBFE_NEWPT_LOW_PARALLAX 0   /* the final `else continue`: no stereo keypoint and too little parallax */
#define ORBFE_NEWPT_W_ZERO 1         /* x3D(3) == 0 after the SVD */
#define ORBFE_NEWPT_DEPTH1 2         /* z1 <= 0; also UnprojectStereo(idx1) with mvDepth <= 0, where the reference throws */
#define ORBFE_NEWPT_DEPTH2 3
#define ORBFE_NEWPT_ERR1 4           /* reprojection error in keyframe 1 above 5.991 (mono) / 7.8 (stereo) * sigma2 */
#define ORBFE_NEWPT_ERR2 5
#define ORBFE_NEWPT_DIST_ZERO 6
#define ORBFE_NEWPT_SCALE 7          /* the scale-consistency gate */
#define ORBFE_NEWPT_OK 8             /* a MapPoint is created */
#define ORBFE_NEWPT_IGNORED 9        /* batch forms: an index >= the keyframe's d_n or an octave outside [0, nlevels) */
typedef struct orbfe_newpt_key {
    float ux, uy;                    /* mvKeysUn[idx].pt */
    float rx, ry;                    /* mvKeys[idx].pt: what KeyFrame::UnprojectStereo reads (= ux, uy without distortion) */
    float depth, uright;             /* mvDepth[idx], mvuRight[idx]: stereo means uright >= 0 */
    int32_t octave;
} orbfe_newpt_key;
/* One match on the HOST, the function the kernel runs (no device, no handle): Tcw row-major 3x4, Ow = GetCameraCenter, both
 * keyframes share `cam` (fx, fy, cx, cy, bf: u2_r uses keyframe 1's mbf in the reference, sic) and mb; scale_factors /
 * level_sigma2 have nlevels entries, scale_factor = mfScaleFactor.  cos(2 * atan2(mb / 2, depth)) is evaluated with the
 * library's canonical trig (DESIGN.md "Canonical trig"), not the host's libm.  Returns ORBFE_NEWPT_*, or -1 for a bad argument
 * (an octave outside the tables included); x3D [3] is the point for ORBFE_NEWPT_OK. */
int32_t orbfe_triangulate_match(const float *Tcw1, const float *Ow1, const float *Tcw2, const float *Ow2, const orbfe_track_camera *cam,
                                float mb, const orbfe_newpt_key *k1, const orbfe_newpt_key *k2, const float *scale_factors,
                                const float *level_sigma2, int32_t nlevels, float scale_factor, float *x3D);
/* what the batch forms read beside the orbfe_tri_keyframes block (whose d_kps are mvKeysUn and whose d_uright they read too) */
typedef struct orbfe_newpt_geom {
    const orbfe_keypoint *d_kps_raw; /* [nframes][cap] mvKeys; NULL = the block's d_kps */
    const float *d_depth;            /* [nframes][cap] mvDepth; may be NULL when d_uright is */
    const float *d_Tcw, *d_Ow;       /* [nframes][12], [nframes][3] */
    orbfe_track_camera cam;
    float mb, scale_factor;
} orbfe_newpt_geom;
typedef struct orbfe_newpt_out {
    uint8_t *d_verdict;              /* [npairs][cap]: ORBFE_NEWPT_* of entry j of d_pairs; entries past d_npairs[p] keep what they held */
    int32_t *d_new_idx;              /* [npairs][cap][2] (idx1, idx2) of the accepted matches, in vMatchedIndices order = the order
                                      * `new MapPoint` runs in; rows past d_nnew[p] keep what they held */
    float *d_new_xyz;                /* [npairs][cap][3] their world positions */
    int32_t *d_nnew;                 /* [npairs] */
} orbfe_newpt_out;
/* All matches of npairs pairs: d_pairs / d_npairs as orbfe_search_for_triangulation_batch_device writes them.  Counts are clamped
 * into [0, cap]; a pair with a frame index outside the block gets 0 points; an entry with an index >= the keyframe's d_n or a
 * keypoint whose octave is outside [0, nlevels) gets ORBFE_NEWPT_IGNORED (it cannot be rejected without a host read).  Ordered
 * compaction, no atomic takes a slot.  Enqueued on `stream`: no wait, no host writes; scratch is the matcher's.  scale_factors /
 * level_sigma2 are HOST arrays.  Limits: those of the batched search. */
orbfe_status orbfe_triangulate_pairs_batch_device(orbfe_matcher *m, const orbfe_tri_keyframes *kf, const orbfe_newpt_geom *geom,
                                                  const int32_t *d_kf1, const int32_t *d_kf2, int32_t npairs, const int32_t *d_pairs,
                                                  const int32_t *d_npairs, const float *scale_factors, const float *level_sigma2,
                                                  int32_t nlevels, const orbfe_newpt_out *out, void *stream);
/* KeyFrame::ComputeSceneMedianDepth(q) of every keyframe of the block, one workgroup each: z = (float)(Tcw.row(2).dot(x) + Tcw(2, 3))
 * over the occupied slots (d_has_mp != 0, slot < d_n clamped into [0, cap]), d_median[f] = the ((count - 1) / q)-th smallest,
 * selected exactly (radix selection on order-preserving keys).  A keyframe with no MapPoint is undefined behaviour in the
 * reference; THIS LIBRARY writes -1.0f, which the monocular baseline gate turns into a skipped pair.  d_mp_xyz [nframes][cap][3].
 * cap <= 8192, q >= 1. */
orbfe_status orbfe_scene_median_depth_batch_device(orbfe_matcher *m, const float *d_Tcw, const uint8_t *d_has_mp, const float *d_mp_xyz,
                                                   const int32_t *d_n, int32_t nframes, int32_t cap, int32_t q, float *d_median,
                                                   void *stream);
/* the slot state CreateNewMapPoints changes, beside the keyframe block */
typedef struct orbfe_newpt_state {
    uint8_t *d_has_mp;               /* [nframes][cap] */
    float *d_mp_xyz;                 /* [nframes][cap][3] */
    int32_t *d_mp_id;                /* [nframes][cap]: -1 none, else the id of the slot's MapPoint (the caller's for its own points) */
} orbfe_newpt_state;
/* The neighbour loop with carried state.  The pairs arrive in round order; round r is the pairs round_off[r] .. round_off[r + 1]
 * (a HOST array of nrounds + 1 ascending offsets, round_off[nrounds] = npairs).  Per round, on `stream`, without a host read:
 * with `mono` the median depth (q = 2) of the round's keyframes 2 from the current state, orbfe_triangulation_pairs_batch_device,
 * orbfe_search_for_triangulation_batch_device with the current d_has_mp (kf->d_has_mp is ignored), the triangulation above, and
 * the claim: accepted point k of pair p has the id id_base + p * cap + k (ascending in creation order), each of its two slots takes
 * the MAXIMUM id that claims it -- the reference's AddMapPoint leaves the last one created in a slot -- then d_has_mp = 1 and the
 * winner's position.  Every pair of a round sees the state at the start of its round: the result equals the reference's serial
 * loop whenever no keyframe occurs in two pairs of one round (orbfe_newpoints_plan_rounds), and nrounds == 1 is the static
 * batch.  d_pair_skip [npairs] may be NULL.  Outputs are indexed by the pair's position in the given (round) order. */
orbfe_status orbfe_create_new_map_points_batch_device(orbfe_matcher *m, const orbfe_tri_keyframes *kf, const orbfe_newpt_geom *geom,
                                                      const orbfe_newpt_state *state, int32_t mono, const int32_t *d_kf1,
                                                      const int32_t *d_kf2, int32_t npairs, const int32_t *round_off, int32_t nrounds,
                                                      const float *scale_factors, const float *level_sigma2, int32_t nlevels,
                                                      int32_t th_low, int32_t only_stereo, int32_t check_ori, int32_t id_base,
                                                      uint8_t *d_pair_skip, const orbfe_tri_out *tri_out, const orbfe_newpt_out *out,
                                                      void *stream);
/* bytes of matcher scratch the two calls above take beside the search's; -1 outside the limits.  No device needed. */
int64_t orbfe_newpoints_scratch_bytes(int32_t npairs, int32_t cap, int32_t nframes);
/* The GPU-free planner (host): round_of[i] = the earliest round later than the round of every earlier pair that shares a keyframe
 * with pair i (pairs with disjoint keyframes commute, pairs that share one keep their order); order[j] = the pair that stands at
 * position j in round order (a stable permutation); round_off[0 .. nrounds].  round_of / order: npairs entries, round_off:
 * npairs + 1.  Returns nrounds, or -1 for a bad argument. */
int32_t orbfe_newpoints_plan_rounds(const int32_t *kf1, const int32_t *kf2, int32_t npairs, int32_t *round_of, int32_t *order,
                                    int32_t *round_off);

/* Fuse, batched: ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:1031-1182; LocalMapping::SearchInNeighbors, once per
 * target keyframe and once more with every target's points against the current keyframe) and Fuse(pKF, Scw, vpPoints, th,
 * vpReplacePoint) (:1198-1318; LoopClosing::SearchAndFuse) for a batch of (keyframe, list of MapPoints) pairs, device-resident
 * (csrc/orbfe_fuse.hip; the gate is csrc/orbfe_track_geom.h's trk_gate_fuse, host and device alike).
 *
 * Pair p fuses the list d_list_idx[d_list_off[p] .. d_list_off[p + 1]) (indices into `map`, CSR over all pairs) into keyframe row
 * d_pair_kf[p] of an orbfe_track_frames block (keypoint records read in place, the grid of orbfe_assign_grid_batch_device; d_uright
 * drives the stereo branch of the reprojection gate, NULL = every keypoint is monocular; d_slot is not read).  The same keyframe
 * may stand in many pairs.  The pose is per PAIR: d_Tcw[p][12] row-major 3x4 (Rcw | tcw) and d_Ow[p][3]; pose-level expressions
 * stay the caller's -- Ow = GetCameraCenter(), and for the Sim3 overload Rcw = sRcw / scw, tcw = Scw.col(3) / scw, Ow = -Rcw.t() *
 * tcw.  cam->minx .. maxy are KeyFrame::mnMinX .. mnMaxY.
 *
 * Per entry, in the reference's order (rules F1 .. of DESIGN.md 8p): a negative index is a NULL pointer, map->d_bad is isBad() at
 * entry and a non-zero d_list_skip byte (may be NULL) is the dynamic reason the reference `continue`s on -- IsInKeyFrame(pKF) /
 * spAlreadyFound.count(pMP); then p3Dc = Rcw * p3Dw + tcw, z < 0 out, invz = 1 / z, u = fx * (X * invz) + cx, KeyFrame::IsInImage
 * (min <= u < max; a NaN from z == 0 is out), dist3D = |p3Dw - Ow| outside [0.8f * mfMinDistance, 1.2f * mfMaxDistance] out (the
 * getters' values), PO . Pn < 0.5 * dist3D (in double) out, level = PredictScale from the UNSCALED mfMaxDistance (src/MapPoint.cc:
 * 448-463) -- so for these calls map->d_min_dist / d_max_dist hold mfMinDistance / mfMaxDistance themselves and the gate applies
 * the getters' factors --, GetFeaturesInArea(u, v, th * scale_factors[level]), candidates of octave level - 1 or level, in the PLAIN
 * overload the chi2 gate of ORBFE_PROJ_CHI2_GATE, the FIRST candidate in GetFeaturesInArea order with the smallest Hamming distance
 * (`dist < bestDist`), accepted iff bestDist <= th_low.  That result depends on the point, the pose and the keyframe's features
 * only -- never on what another entry or an earlier Fuse call did to the map.
 * Three things cannot be rejected without a host read and make "no match": a list index >= map->npoints, a pair whose keyframe row
 * is outside [0, nkf), and a keypoint whose octave is outside [0, nlevels) (it is never a candidate).  Offsets beyond nentries are
 * cut there.  Limits: cap <= 15360, nlevels <= 16, 0 <= th_low <= 255, nentries <= 2^25; anything else is ORBFE_ERR_ARG before any
 * launch. */
#define ORBFE_FUSE_PLAIN 0
#define ORBFE_FUSE_SIM3 1
/* what the reference does with an entry (d_action) */
#define ORBFE_FUSE_NONE 0               /* no match */
#define ORBFE_FUSE_ADD 1                /* the slot is empty and this entry is its first match: AddObservation + AddMapPoint */
#define ORBFE_FUSE_REPLACE_SLOT 2       /* plain: the slot's point is good and does not have more observations (equal counts land
                                         * here): pMPinKF->Replace(pMP); d_other = the slot's point */
#define ORBFE_FUSE_REPLACE_POINT 3      /* plain: the slot's point is good and has more observations: pMP->Replace(pMPinKF) */
#define ORBFE_FUSE_COUNTED 4            /* the slot's point is bad: only nFused++ (such a slot never changes) */
#define ORBFE_FUSE_DEFERRED 5           /* plain: an earlier entry of this pair matched the same slot with action 1, 2 or 3; what the
                                         * reference does now depends on what Replace / AddObservation did to the map (observation
                                         * transfers across keyframes, +2 for a stereo keypoint), which flat arrays cannot express:
                                         * the caller decides it in list order; d_other = the in-pair position of that first matcher */
#define ORBFE_FUSE_REPLACE_CANDIDATE 6  /* Sim3: vpReplacePoint[i] = d_other: the slot's point at entry if it is good, else the
                                         * point an earlier entry of this call ADDed to the slot (Replace is the caller's there, so the
                                         * replay is complete: no DEFERRED in this overload) */
typedef struct orbfe_fuse_lists {
    const int32_t *d_pair_kf;        /* [npairs] row of the keyframe block */
    const float *d_Tcw;              /* [npairs][12] */
    const float *d_Ow;               /* [npairs][3] */
    const uint32_t *d_list_off;      /* [npairs + 1] ascending */
    const int32_t *d_list_idx;       /* [nentries] map index, negative = NULL */
    const uint8_t *d_list_skip;      /* [nentries] or NULL */
    int64_t nentries;
    int32_t npairs;
} orbfe_fuse_lists;
/* flat, aligned with the CSR list; d_first may be NULL */
typedef struct orbfe_fuse_out {
    int32_t *d_match;                /* [nentries] bestIdx of an accepted entry, else -1 */
    int32_t *d_dist;                 /* [nentries] bestDist, 256 = no candidate */
    uint8_t *d_action;               /* [nentries] ORBFE_FUSE_* */
    int32_t *d_other;                /* [nentries] map index of the other point (2, 3, 6), position of the first matcher (5), else -1 */
    int32_t *d_nfused;               /* [npairs] the reference's return value: every accepted entry counts */
    int32_t *d_first;                /* [npairs][cap] per slot the smallest in-pair position that matched it, -1 none */
} orbfe_fuse_out;
/* the gate and the search alone: d_match / d_dist [nentries].  map->d_obs_gt0 is not read.  scale_factors / inv_level_sigma2 are
 * HOST arrays of nlevels floats (mvScaleFactors / mvInvLevelSigma2), log_scale_factor = mfLogScaleFactor.  Takes no scratch. */
orbfe_status orbfe_fuse_search_batch_device(orbfe_matcher *m, const orbfe_track_frames *kf, int32_t nkf, const orbfe_fuse_lists *lists,
                                            const orbfe_track_camera *cam, const orbfe_track_map *map, float th,
                                            const float *scale_factors, const float *inv_level_sigma2, int32_t nlevels,
                                            float log_scale_factor, int32_t th_low, int32_t mode, int32_t *d_match, int32_t *d_dist,
                                            void *stream);
/* search + replay.  The slot state is flat and READ ONLY: d_slot_mp [nkf][cap] = -1 (no MapPoint) or the map index of
 * GetMapPoint(slot) (NULL: every slot is empty; an index >= map->npoints counts as empty), d_nobs [npoints] = Observations()
 * (plain overload).  Every pair is replayed against the state AT ENTRY.  The caller owns two cases: the same point twice in one
 * list (the second occurrence is replayed as if it were another point), and the later Fuse calls of a loop after an earlier one
 * changed the map.  Since d_match never depends on either, a caller that replays all pairs in order on its own graph using d_match
 * gets the reference's result; d_action saves it the work wherever the entry state decides.  Enqueued on `stream`, waits for nothing,
 * writes no host memory. */
orbfe_status orbfe_fuse_batch_device(orbfe_matcher *m, const orbfe_track_frames *kf, int32_t nkf, const orbfe_fuse_lists *lists,
                                     const orbfe_track_camera *cam, const orbfe_track_map *map, const int32_t *d_nobs,
                                     const int32_t *d_slot_mp, float th, const float *scale_factors, const float *inv_level_sigma2,
                                     int32_t nlevels, float log_scale_factor, int32_t th_low, int32_t mode, const orbfe_fuse_out *out,
                                     void *stream);
/* trk_gate_fuse on the HOST for n points of one pair (no device, no handle): q[n] the query (r = th * scale_factors[level], levels
 * [level - 1, level], ur = u - bf * invz, flags ORBFE_PROJ_CHI2_GATE for ORBFE_FUSE_PLAIN and 0 for ORBFE_FUSE_SIM3), level[n], ok[n];
 * zeros and level -1 where ok is 0.  min_dist / max_dist are mfMinDistance / mfMaxDistance.  Bit for bit what orbfe_project_points
 * (ORBFE_PJ_SKIP_NEG_DEPTH, open upper bounds) gives when it is handed the getters' 0.8f * min_dist / 1.2f * max_dist. */
orbfe_status orbfe_fuse_gate_points(const float *Tcw, const float *Ow, const orbfe_track_camera *cam, float th, const float *scale_factors,
                                    float log_scale_factor, int32_t nlevels, int32_t mode, int32_t n, const float *world_pos,
                                    const float *normal, const float *min_dist, const float *max_dist, orbfe_proj_query *q,
                                    int32_t *level, uint8_t *ok);
/* vpFuseCandidates of SearchInNeighbors (src/LocalMapping.cc:705-725) from the slot state: the map indices of the occupied slots
 * (slot < d_n[kf] clamped into [0, cap]) of the target keyframe rows d_targets[ntargets], in (target, slot) order; bad points are
 * dropped first, then every occurrence after the first (the mnFuseCandidateForKF stamp).  Ordered: no atomic takes an output place.
 * d_cand [cand_cap]; d_ncand[0] = entries written, d_ncand[1] = the full count.  With cur_kf >= 0 and d_cand_skip [cand_cap] != NULL,
 * d_cand_skip[j] = candidate j already sits in a slot of keyframe row cur_kf (IsInKeyFrame): the d_list_skip of the last Fuse of
 * SearchInNeighbors, without reading the list back.  A target row outside [0, nkf) has no points.  Limits: cap <= 15360, ntargets *
 * cap < 2^25. */
orbfe_status orbfe_fuse_candidates_device(orbfe_matcher *m, const int32_t *d_slot_mp, const int32_t *d_n, int32_t nkf, int32_t cap,
                                          const int32_t *d_targets, int32_t ntargets, int32_t cur_kf, const uint8_t *d_bad,
                                          int32_t npoints, int32_t *d_cand, uint8_t *d_cand_skip, int32_t cand_cap, int32_t *d_ncand,
                                          void *stream);
/* bytes of matcher scratch orbfe_fuse_candidates_device takes (the search and the replay take none); -1 outside the limits.  No
 * device needed. */
int64_t orbfe_fuse_scratch_bytes(int32_t npoints, int32_t ntargets, int32_t cap);

/* SearchBySim3 and the loop's SearchByProjection, batched: the two ORBmatcher members LoopClosing::ComputeSim3 calls between
 * Sim3Solver::iterate and SearchAndFuse -- SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/ORBmatcher.cc:1334-1558)
 * and SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (:378-498) -- for a batch of loop candidates, device-resident
 * (csrc/orbfe_sim3_search.hip; the per-point arithmetic is csrc/orbfe_track_geom.h's trk_sim3_pair_pose / trk_gate_sim3 /
 * trk_gate_fuse, host and device alike).  Conventions of the Fuse calls: everything is enqueued on `stream`, no call
 * waits for the device or writes host memory, scratch is the matcher's, keyframes are rows of an orbfe_track_frames block with the
 * grid of orbfe_assign_grid_batch_device (d_uright and d_slot are not read), map->d_min_dist / d_max_dist hold mfMinDistance /
 * mfMaxDistance and the gates apply the getters' 0.8f / 1.2f, scale_factors is a HOST array of nlevels floats.  Limits: cap <=
 * 15360, nlevels <= 16, thresholds 0..255; anything else is ORBFE_ERR_ARG before any launch.
 *
 * The poses (:1355-1357) as row-major 3x4 blocks T12 = (sR12 | t12), T21 = (sR21 | t21): sR12 = (float)(R12[i] * (double)s12),
 * sR21 = (float)(R12^T[i] * (1.0 / (double)s12)), t21 = (-sR21) * t12 as a float matrix product accumulated from 0 left to right.
 * orbfe_sim3_pair_pose: one candidate on the HOST (no device, no handle).  orbfe_sim3_pair_poses_device: one thread per candidate;
 * candidate p's record starts at d_src + p * stride (bytes) and holds the scale (one float at off_s), the rotation (9 floats at
 * off_R, row-major) and the translation (3 floats at off_t) -- the model.s / model.R / model.t of an orbfe_sim3_result read in
 * place, or a plain [s, R, t] array with stride 52 and offsets 0, 4, 40; off_found >= 0 names an int32 of the record (the
 * result's `found`): where it is 0 the candidate gets zeros in both poses and d_pair_skip[p] = 1 (else 0; may be NULL), the byte
 * the searches below take as "this pair does nothing".  stride and offsets are multiples of 4. */
orbfe_status orbfe_sim3_pair_pose(float s12, const float *R12, const float *t12, float *T12, float *T21);
orbfe_status orbfe_sim3_pair_poses_device(orbfe_matcher *m, const void *d_src, int64_t stride, int32_t off_s, int32_t off_R,
                                          int32_t off_t, int32_t off_found, int32_t npairs, float *d_T12, float *d_T21,
                                          uint8_t *d_pair_skip, void *stream);
/* trk_gate_sim3 on the HOST for n points of one direction (no device, no handle; :1400-1431 / :1476-1503): pc = T_own * Pw with
 * the pose (Rcw | tcw) of the keyframe that holds the points, pc' = T_to_other * pc with (sR21 | t21) or (sR12 | t12); pc'.z < 0
 * out; invz = 1 / z, u = fx * (x * invz) + cx; KeyFrame::IsInImage (min <= u < max; NaN is out); dist3D = |pc'| (the camera-frame
 * point, a double sum of squares) outside [0.8f * min_dist, 1.2f * max_dist] out; no viewing-angle gate; level = PredictScale from
 * the unscaled max_dist.  q[n]: r = th * scale_factors[level], levels [level - 1, level], ur = u - bf * invz, flags 0; level[n],
 * ok[n]; zeros and level -1 where ok is 0. */
orbfe_status orbfe_sim3_gate_points(const float *T_own, const float *T_to_other, const orbfe_track_camera *cam, float th,
                                    const float *scale_factors, float log_scale_factor, int32_t nlevels, int32_t n,
                                    const float *world_pos, const float *min_dist, const float *max_dist, orbfe_proj_query *q,
                                    int32_t *level, uint8_t *ok);
/* SearchBySim3 for npairs candidates: pair p = (keyframe rows d_kf1[p], d_kf2[p]) of `kf` (the same keyframe may stand in many
 * pairs, on either side), poses d_Tcw [nkf][12], slot table d_slot_mp [nkf][cap] as in orbfe_fuse_batch_device (map index or -1; an
 * index >= map->npoints counts as empty), similarity d_T12 / d_T21 [npairs][12], d_pair_skip [npairs] or NULL.  map->d_normal and
 * d_obs_gt0 are not read.  d_match12 [npairs][cap] is vpMatches12 in / out in INDEX form (what orbfe_search_by_bow_batch_device
 * yields after inversion): -1 NULL, j >= 0 the point in slot j of keyframe 2, -2 a point keyframe 2 does not observe; so
 * vbAlreadyMatched1[i] = d_match12[p][i] != -1 and vbAlreadyMatched2[j] for every 0 <= j < N2 in the row.  Both directions gate
 * with one thread per slot, compact the live queries and search with one wave per live query: the FIRST candidate in
 * GetFeaturesInArea order with the smallest distance among the octaves level - 1 and level, accepted iff <= th_high; an already
 * matched feature of the other keyframe stays a candidate.  Then the agreement pass (:1542-1555): d_match12[p][i1] = idx2 where
 * vnMatch1[i1] == idx2 and vnMatch2[idx2] == i1; d_nfound[p] = the return value.  d_match1 / d_match2 [npairs][cap] (may be NULL):
 * vnMatch1 / vnMatch2, -1 elsewhere up to cap.  A pair with a keyframe row outside [0, nkf) or with a skip byte gets d_nfound[p] =
 * 0 and its d_match12 row stays as it was.  Further limit: npairs * 2 * cap < 2^25. */
orbfe_status orbfe_search_by_sim3_batch_device(orbfe_matcher *m, const orbfe_track_frames *kf, int32_t nkf, const float *d_Tcw,
                                               const int32_t *d_slot_mp, const orbfe_track_map *map, const orbfe_track_camera *cam,
                                               const int32_t *d_kf1, const int32_t *d_kf2, const float *d_T12, const float *d_T21,
                                               const uint8_t *d_pair_skip, int32_t npairs, float th, int32_t th_high,
                                               const float *scale_factors, int32_t nlevels, float log_scale_factor, int32_t *d_match12,
                                               int32_t *d_nfound, int32_t *d_match1, int32_t *d_match2, void *stream);
/* d_list_skip[e] = 1 where the point of list entry e (d_list_idx, CSR over the pairs by d_list_off, as orbfe_fuse_lists) stands
 * anywhere in row d_pair_row[p] (NULL: row p) of d_rows [nrows][cap], else 0: spAlreadyFound.count(pMP) with the rows = vpMatched,
 * IsInKeyFrame(pKF) -- Fuse's d_list_skip -- with the rows = the slot table.  Negative row values and negative list indices are
 * members of nothing; a row outside [0, nrows) has no members.  Exact and deterministic; takes no scratch.  nentries <= 2^25. */
orbfe_status orbfe_mark_list_members_device(orbfe_matcher *m, const int32_t *d_rows, int32_t nrows, int32_t cap,
                                            const int32_t *d_pair_row, const uint32_t *d_list_off, const int32_t *d_list_idx,
                                            int64_t nentries, int32_t npairs, uint8_t *d_list_skip, void *stream);
/* SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) for npairs (keyframe, list) pairs: pair p searches keyframe row p of `kf`
 * (one keyframe under two poses: pass its row twice) under the pose d_Tcw[p][12], d_Ow[p][3] -- the caller's pose-level
 * expressions, as for Fuse's Sim3 overload -- with the list d_list_idx[d_list_off[p] .. d_list_off[p + 1]) of map indices (an index
 * outside [0, map->npoints) makes no query).  d_matched [npairs][cap] is vpMatched in / out: the map index of the point, -1 NULL
 * (any other value is a point that is in no list).  (a) a list entry whose point stands in d_matched[p] AT ENTRY is skipped
 * (orbfe_mark_list_members_device, or the caller's d_list_skip [nentries] when not NULL); (b) the gate is Fuse's Sim3 gate
 * (trk_gate_fuse without chi2), the queries leave compacted in list order, at most qcap per pair (qcap >= the longest list always
 * suffices; queries past it are dropped); (c) the search is the batch core of orbfe_search_by_projection_batch_device: slots
 * occupied at entry are never candidates, an accepted query's slot is skipped by every later one, no ratio rule, accepted iff
 * bestDist <= th_low; ent_cap / d_status [2] as there -- when ent_cap is too small d_status[0] holds the exact need, d_matched
 * stays as it was and d_nmatches is 0: call again; (d) d_matched[p][bestIdx] = the point, d_nmatches[p] = the return value.
 * Further limits: npairs * qcap < 2^25, nentries <= 2^25. */
orbfe_status orbfe_search_by_projection_sim3_batch_device(orbfe_matcher *m, const orbfe_track_frames *kf, int32_t npairs,
                                                          const float *d_Tcw, const float *d_Ow, const orbfe_track_camera *cam,
                                                          const orbfe_track_map *map, const uint32_t *d_list_off,
                                                          const int32_t *d_list_idx, const uint8_t *d_list_skip, int64_t nentries,
                                                          float th, const float *scale_factors, int32_t nlevels, float log_scale_factor,
                                                          int32_t th_low, int32_t qcap, int64_t ent_cap, int32_t *d_matched,
                                                          int32_t *d_nmatches, int32_t *d_status, void *stream);
/* bytes of matcher scratch: qcap == 0 -- orbfe_search_by_sim3_batch_device for (npairs, cap); qcap >= 1 --
 * orbfe_search_by_projection_sim3_batch_device for (npairs, cap, qcap, nentries, ent_cap), the batch core's blocks included.  -1
 * outside the limits.  No device needed. */
int64_t orbfe_sim3_search_scratch_bytes(int32_t npairs, int32_t cap, int32_t qcap, int64_t nentries, int64_t ent_cap);
/* The glue of one ComputeSim3 round on one stream, between orbfe_search_by_bow_batch_device(kf_kf = 1), orbfe_sim3_iterate_device and
 * orbfe_search_by_sim3_batch_device; pair p = (keyframe rows d_kf1[p], d_kf2[p]), every row [npairs][cap].
 * orbfe_sim3_invert_matches_device: d_bow_match[p][i] = the keyframe-1 feature SearchByBoW assigned to keyframe-2 feature i (-1 none)
 *   -> d_match12[p][i1] = that i (vpMatches12 in index form), -1 elsewhere up to cap; i < d_n[d_kf2[p]].
 * orbfe_sim3_correspondences_device: Sim3Solver's constructor (src/Sim3Solver.cc:43-115) for every pair, as the CSR
 *   orbfe_sim3_iterate_device takes: in i1 order every d_match12[p][i1] = j in [0, N2) whose two slots hold good points (d_slot_mp,
 *   map->d_bad; keypoint octaves inside [0, nlevels)) gives X1 = Rcw1 * Xw1 + tcw1, X2 likewise (orbfe_sim3_prepare_device's
 *   arithmetic, the poses read from d_Tcw [nkf][12]), sigma2_1 / sigma2_2 = level_sigma2[octave] (HOST array, mvLevelSigma2) and
 *   d_idx1 = i1 (mvnIndices1); d_offsets [npairs + 1].  corr_cap entries of every output, corr_cap >= npairs * cap.  Ordered: no atomic
 *   takes a place.  Takes 4 * npairs bytes of matcher scratch.
 * orbfe_sim3_keep_inliers_device: d_match12[p][i1] = -1 where d_key_mask[p * cap + i1] == 0 -- iterate's vbInliers with every set's
 *   key_offset = p * cap and n_keys = cap (src/LoopClosing.cc:410-416). */
orbfe_status orbfe_sim3_invert_matches_device(orbfe_matcher *m, const int32_t *d_bow_match, const int32_t *d_kf2, const int32_t *d_n,
                                              int32_t nkf, int32_t cap, int32_t npairs, int32_t *d_match12, void *stream);
orbfe_status orbfe_sim3_correspondences_device(orbfe_matcher *m, const orbfe_track_frames *kf, int32_t nkf, const float *d_Tcw,
                                               const int32_t *d_slot_mp, const orbfe_track_map *map, const int32_t *d_kf1,
                                               const int32_t *d_kf2, int32_t npairs, const int32_t *d_match12, const float *level_sigma2,
                                               int32_t nlevels, int32_t corr_cap, int32_t *d_offsets, float *d_X1, float *d_X2,
                                               float *d_sigma2_1, float *d_sigma2_2, int32_t *d_idx1, void *stream);
orbfe_status orbfe_sim3_keep_inliers_device(orbfe_matcher *m, const uint8_t *d_key_mask, int32_t cap, int32_t npairs, int32_t *d_match12,
                                            void *stream);

/* Frame::ComputeStereoMatches (src/Frame.cc:642-846): row-band descriptor search in the right image,
 * 11 x 11 SAD refinement over 11 shifts on the two extractors' device-resident pyramids (mvImagePyramid of the LAST
 * call of `left` / `right`, frame 0), parabola fit, disparity -> depth, and the median-based outlier rejection.
 *   kpsL/descL/nL, kpsR/descR/nR  what those two calls returned (mvKeys / mDescriptors, mvKeysRight / mDescriptorsRight)
 *   mbf, mb                       baseline * fx and the baseline; the reference reads mb before assigning it (:682,
 *                                 undefined) -- here minZ = mb is an explicit argument
 *   uRight[nL], depth[nL]         mvuRight / mvDepth, -1 where no match.  HOST buffers.
 * The two extractors must have the same level count, scale factors and level sizes (as the reference's stereo Frame,
 * whose two extractors share its settings and image size); ORBFE_ERR_ARG otherwise.  So must the batched form below. */
orbfe_status orbfe_stereo_matches(orbfe_matcher *m, orbfe_handle *left, orbfe_handle *right, const orbfe_keypoint *kpsL,
                                  const uint8_t *descL, int32_t nL, const orbfe_keypoint *kpsR, const uint8_t *descR,
                                  int32_t nR, float mbf, float mb, float *uRight, float *depth);

/* The same for a whole batch, without leaving the device: frame pair f = frame f of the LAST orbfe_extract_batch_device
 * call of `left` and of `right` (the stereo Frame constructor runs the two extractors side by side, src/Frame.cc:82-87),
 * their output blocks exactly as those calls wrote them -- d_kps* [nframes][cap], d_desc* [nframes][cap][32], d_n*
 * [nframes] -- and d_uRight / d_depth [nframes][cap] floats (slots >= the frame's count are left untouched).  Everything
 * is enqueued on `stream` (the stream the two extract calls ran on, or one ordered after it); d_gray of both calls must
 * still be alive.  No host synchronisation. */
orbfe_status orbfe_stereo_matches_batch_device(orbfe_matcher *m, orbfe_handle *left, orbfe_handle *right,
                                               const orbfe_keypoint *d_kpsL, const uint8_t *d_descL, const int32_t *d_nL,
                                               const orbfe_keypoint *d_kpsR, const uint8_t *d_descR, const int32_t *d_nR,
                                               int32_t cap, int32_t nframes, float mbf, float mb, float *d_uRight,
                                               float *d_depth, void *stream);

/* DBoW2 TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup) as called by
 * Frame::ComputeBoW / KeyFrame::ComputeBoW (src/Frame.cc:553, src/KeyFrame.cc:82; levelsup = 4).  DBoW2 is not vendored
 * by the reference; the algorithm is restated from the published one.  The tree is handed over as arrays:
 * children of node i = child_idx[child_off[i] .. child_off[i+1]) in stored order (node 0 = root; child ids must exceed
 * their parent's id), node_desc[nnodes*32], word_id / weight (TF-IDF) meaningful for leaves, L = tree depth.
 * A leaf's word_id must be below 2^31 (f_word is int32, -1 = no word): ORBFE_ERR_ARG otherwise.
 * A root without children (child_off[1] == child_off[0]; a vocabulary file that holds the header only) is DBoW2's empty()
 * vocabulary: it is accepted, and every transform through it gives "no word" for every feature -- f_word = f_node = -1,
 * f_weight = 0, empty BowVector and FeatureVector (counts 0 / 0 / 0, fv_off[0] = 0) -- in orbfe_bow_transform and in
 * orbfe_bow_transform_batch_device alike; child_idx may then be NULL and is never read. */
typedef struct orbfe_vocabulary orbfe_vocabulary;
orbfe_status orbfe_vocabulary_create(int32_t device, int32_t nnodes, const uint32_t *child_off, const uint32_t *child_idx,
                                     const uint8_t *node_desc, const uint32_t *word_id, const double *weight, int32_t L,
                                     orbfe_vocabulary **out);
void orbfe_vocabulary_destroy(orbfe_vocabulary *v);
/* desc[n*32] (n <= 8192).  Per feature (any may be NULL): f_word / f_node (-1 when the word's weight is 0 and the feature
 * is skipped) / f_weight.  BowVector: bow_id[<= n] ascending, bow_val L1-normalised doubles, *nbow.  FeatureVector as the
 * CSR orbfe_search_by_bow takes: fv_node[<= n] ascending, fv_off[*nfv + 1], fv_idx[<= n].  HOST buffers. */
orbfe_status orbfe_bow_transform(orbfe_matcher *m, const orbfe_vocabulary *v, const uint8_t *desc, int32_t n,
                                 int32_t levelsup, int32_t *f_word, int32_t *f_node, double *f_weight, uint32_t *bow_id,
                                 double *bow_val, int32_t *nbow, uint32_t *fv_node, uint32_t *fv_off, uint32_t *fv_idx,
                                 int32_t *nfv);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:284-345) for a batch of map points.
 *   pool[npool*32]      descriptors (rows of the observing keyframes' mDescriptors)
 *   off[npoints+1], idx map point p observes pool[idx[off[p] .. off[p+1])]  (at most 1024 observations per point)
 *   best_idx[npoints]   position inside the point's list of the descriptor with the least median Hamming distance to
 *                       the others (self distance 0 included, element (int)(0.5*(N-1)) of the sorted row; first on
 *                       ties); median[npoints] that median; both -1 for a point without observations.  HOST buffers. */
orbfe_status orbfe_distinctive_descriptors(orbfe_matcher *m, const uint8_t *pool, int32_t npool, const uint32_t *off,
                                           const uint32_t *idx, int32_t npoints, int32_t *best_idx, int32_t *median);

/* The same on device buffers (the pool is typically the all-gathered descriptor block of the keyframes: observation index
 * = keyframe * cap + slot): nothing is validated or copied, the launch goes to `stream`.  max_obs (1..1024) sizes the
 * kernel's LDS; a point with more observations than that gets -2 / -2 instead of a result. */
orbfe_status orbfe_distinctive_descriptors_device(orbfe_matcher *m, const uint8_t *d_pool, const uint32_t *d_off,
                                                  const uint32_t *d_idx, int32_t npoints, int32_t max_obs,
                                                  int32_t *d_best_idx, int32_t *d_median, void *stream);

/* ---- the same chain DEVICE-RESIDENT and BATCHED: extractor output block -> BoW -> SearchByBoW, one stream, no host
 * round trip (Frame::ComputeBoW src/Frame.cc:546-555 / KeyFrame::ComputeBoW src/KeyFrame.cc:74-84, then
 * ORBmatcher::SearchByBoW src/ORBmatcher.cc:217-363 / :665-812 for a batch of (KeyFrame, Frame) pairs).
 *
 * orbfe_bow_transform_batch_device: frame b owns `cap` slots of every array (cap + 1 of d_fv_off, 4 of d_counts):
 *   in : d_desc [B][cap][32], d_n [B]               (what orbfe_extract_batch_device wrote; cap <= 8192)
 *   out: d_f_word / d_f_node [B][cap] (-1 = no word / padding), d_f_weight [B][cap] doubles,
 *        d_bow_id / d_bow_val [B][cap]  BowVector, ascending ids, L1-normalised,
 *        d_fv_node [B][cap], d_fv_off [B][cap+1], d_fv_idx [B][cap]  FeatureVector CSR,
 *        d_counts [B][4] = {nbow, nfv, number of indexed features, 0}
 * orbfe_search_by_bow_batch_device: pair p = (KeyFrame d_kf[p], Frame d_f[p]), frame indices into the same blocks;
 *   d_valid [B][cap] (1 = good MapPoint) or NULL = all; kf_kf = 0: SearchByBoW(KeyFrame*, Frame&) (`<= th_low`, d_valid
 *   applies to the KeyFrame side only), kf_kf = 1: SearchByBoW(KeyFrame*, KeyFrame*) (`< th_low`, both sides);
 *   d_match [P][cap]: KF feature index assigned to F feature i (-1 none; for kf_kf invert to get vpMatches12),
 *   d_nmatches [P].  Both calls only enqueue on `stream` (NULL = HIP's default stream). */
orbfe_status orbfe_bow_transform_batch_device(orbfe_matcher *m, const orbfe_vocabulary *v, const uint8_t *d_desc,
                                              const int32_t *d_n, int32_t nframes, int32_t cap, int32_t levelsup,
                                              int32_t *d_f_word, int32_t *d_f_node, double *d_f_weight,
                                              uint32_t *d_bow_id, double *d_bow_val, uint32_t *d_fv_node,
                                              uint32_t *d_fv_off, uint32_t *d_fv_idx, int32_t *d_counts, void *stream);
orbfe_status orbfe_search_by_bow_batch_device(orbfe_matcher *m, const orbfe_keypoint *d_kps, const uint8_t *d_desc,
                                              int32_t cap, const uint8_t *d_valid, const uint32_t *d_fv_node,
                                              const uint32_t *d_fv_off, const uint32_t *d_fv_idx, const int32_t *d_counts,
                                              const int32_t *d_kf, const int32_t *d_f, int32_t npairs, float nnratio,
                                              int32_t th_low, int32_t kf_kf, int32_t check_ori, int32_t *d_match,
                                              int32_t *d_nmatches, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Sequence pipeline: the frame loop of the reference's drivers (perfect/Examples/RGB-D/rgbd_tum.cc:77-119: every frame of
 * the sequence through the Frame constructor = ORBextractor::operator(), then matched against its predecessor -- BASELINE
 * config 3) for a device-resident SEQUENCE in one call.
 *
 * A pipeline owns `npipes` pipes; a pipe = one extractor handle + one matcher handle on one of the pipeline's streams.  The
 * pipeline creates no more kernel streams than the process has hardware queues (GPU_MAX_HW_QUEUES, read once, default 4:
 * streams that share a queue cannot overlap and stall each other at every cross-stream wait): with queues >= npipes + 1 every
 * pipe has a stream and the pipes' blur a shared side stream, with fewer the side stream takes one queue and queues - 1 pipes
 * take work.  On exactly 3 kernel streams + side stream (the default 4 queues, more than 3 pipes) a device call of two or more
 * sub-batches deals those four streams by STAGE instead -- pyramid | FAST | quadtree + descriptor + matcher | blur, min(npipes, 8)
 * extractor handles as rotating buffer sets -- so that one FAST pass is in flight nearly all the time (DESIGN.md "Lanes");
 * results, ordering guarantees and orbfe_pipeline_join / _synchronize are the same either way.  A call cuts its
 * nframes into sub-batches of p->max_batch frames (the last one may be shorter) and deals them round robin to those pipes,
 * so that the VALU-bound FAST pass of one sub-batch shares the chip with the HBM / LDS-bound stages of its neighbours
 * (one pipe 273 k, three pipes 302 k frames/s at 1024-frame sub-batches).  Frame k is matched against frame
 * k - 1 as orbfe_match_bf does (best <= th, ratio, rotation histogram) ACROSS sub-batch boundaries; frame 0 of a call is
 * matched against the last frame of the previous call when ORBFE_PIPE_CONTINUE is set (the pipeline keeps its own copy of
 * that frame, the caller may re-use its buffers), otherwise -- and on the first call or after
 * orbfe_pipeline_reset_sequence -- it has no predecessor: its match row is -1, its count 0.
 *   d_gray / d_kps / d_desc / cap / d_n_out   exactly as orbfe_extract_batch_device, for all nframes
 *   d_match [nframes][cap], d_nmatches [nframes]   row k = matches of frame k into frame k - 1 (train index or -1);
 *                                                  d_match == NULL: extract only (BASELINE config 2)
 * The call only enqueues.  The pipes start behind what `stream` holds at the time of the call; unless ORBFE_PIPE_NO_JOIN
 * is set, `stream` is made to wait for all pipes before the call returns, so that anything enqueued on it afterwards sees
 * the results.  With ORBFE_PIPE_NO_JOIN consecutive calls run back to back without draining the chip in between (a
 * throughput loop whose results are consumed later): call orbfe_pipeline_join(pl, stream) or orbfe_pipeline_synchronize(pl)
 * before touching the outputs.  Output blocks re-used by a later call are protected inside the pipeline: every sub-batch records the address ranges
 * it writes, and a later sub-batch waits for the extraction and the matchers of every recorded range that overlaps its own (by
 * address, not by position in the call: shifted base pointers and other call sizes are ordered too).
 * A pipeline is used by one thread at a time.  orbfe_pipeline_extractor / _matcher give the pipes' handles for the per-handle
 * settings (orbfe_set_fast_mode, orbfe_set_profiling, orbfe_matcher_set_bf_kernel) and taps.
 * ------------------------------------------------------------------------------------------- */
typedef struct orbfe_pipeline orbfe_pipeline;
#define ORBFE_PIPE_CONTINUE 1 /* frame 0 continues the sequence of the previous call */
#define ORBFE_PIPE_NO_JOIN 2  /* do not order `stream` behind the pipes at the end of the call */
orbfe_status orbfe_pipeline_create(const orbfe_params *p /* max_batch = frames per sub-batch */, int32_t npipes, orbfe_pipeline **out);
void orbfe_pipeline_destroy(orbfe_pipeline *pl);
int32_t orbfe_pipeline_pipes(const orbfe_pipeline *pl);
int32_t orbfe_pipeline_capacity(const orbfe_pipeline *pl);   /* = orbfe_keypoint_capacity of its handles */
int32_t orbfe_pipeline_sub_batch(const orbfe_pipeline *pl);
orbfe_handle *orbfe_pipeline_extractor(orbfe_pipeline *pl, int32_t pipe);
orbfe_matcher *orbfe_pipeline_matcher(orbfe_pipeline *pl, int32_t pipe);
orbfe_status orbfe_pipeline_extract_match_device(orbfe_pipeline *pl, const uint8_t *d_gray, int32_t nframes, int32_t w, int32_t ht,
                                                 int32_t stride, size_t frame_stride, orbfe_keypoint *d_kps, uint8_t *d_desc,
                                                 int32_t cap, int32_t *d_n_out, int32_t *d_match, int32_t *d_nmatches,
                                                 float nnratio, int32_t th, int32_t check_ori, int32_t flags, void *stream);
/* The same with HOST buffers -- the frame loop as the reference's drivers run it (images from the host, results to the host;
 * BASELINE config 3 as SURVEY 8(d) words it): grays[i] = frame i (w x ht, row pitch stride), results into kps [nframes][cap],
 * desc [nframes][cap][32], n_out [nframes] and, with match != NULL, match [nframes][cap] / nmatches [nframes]; cap >=
 * orbfe_pipeline_capacity().  Chunks of one sub-batch: the H2D copy of chunk c + 1, the pipes of chunk c and the D2H copies of
 * chunk c - 1 overlap (three device buffer sets, two copy streams); consecutive chunks take turns on the pipes.  Page-locked
 * frames / result arrays (hipHostMalloc, hipHostRegister, torch pin_memory) are copied asynchronously as they are; pageable
 * memory works, more slowly.  Blocking: returns when the results are on the host.  ORBFE_PIPE_CONTINUE as above. */
orbfe_status orbfe_pipeline_extract_match(orbfe_pipeline *pl, const uint8_t *const *grays, int32_t nframes, int32_t w, int32_t ht,
                                          int32_t stride, orbfe_keypoint *kps, uint8_t *desc, int32_t cap, int32_t *n_out,
                                          int32_t *match, int32_t *nmatches, float nnratio, int32_t th, int32_t check_ori,
                                          int32_t flags);
/* Pipes the host entry point deals its chunks to (default 1, at most orbfe_pipeline_pipes()).  The host path is bound by the
 * PCIe link, not by the kernels: its chunks should FINISH in order (first in, first out) so that their results leave while
 * the next chunk arrives -- several chunks sharing the chip finish together and stall the copies (measured 172 k frames/s
 * with 1, 156 k with 3, 141 k with 12 on a 57 GB/s link). */
orbfe_status orbfe_pipeline_set_host_pipes(orbfe_pipeline *pl, int32_t n);
/* `stream` waits (at stream level) for everything the pipes hold */
orbfe_status orbfe_pipeline_join(orbfe_pipeline *pl, void *stream);
/* the host waits for the pipes */
orbfe_status orbfe_pipeline_synchronize(orbfe_pipeline *pl);
/* the next call starts a new sequence even with ORBFE_PIPE_CONTINUE */
orbfe_status orbfe_pipeline_reset_sequence(orbfe_pipeline *pl);
/* OR of orbfe_get_overflow over the pipes' extractors (waits for them) */
orbfe_status orbfe_pipeline_get_overflow(orbfe_pipeline *pl, int32_t *flags);

/* ---------------------------------------------------------------------------------------------
 * Batched keyframe mode over several devices (north star: "shards independent frames across the 8 GPUs of one
 * node with an RCCL all-gather of descriptors over xGMI", host stays C++).
 *
 * A batch of nframes independent frames is cut into contiguous shards, shard r on rank r.  orbfe_group_shard_range is the
 * SINGLE source of truth for the cut: every rank gets nframes / world frames and the first nframes % world ranks one more
 * (10 frames over 4 ranks: 3, 3, 2, 2 -- not ceil-sized shards with a short last one); a caller that shards the frames
 * itself (orbfe_group_extract_shard_device) must use it.  Every rank owns three padded blocks for the WHOLE batch -- counts
 * [F], keypoints [F][cap], descriptors [F][cap][32], F = world * shard with shard = ceil(max_batch / world) slots per rank;
 * rank r's frames sit at block indices r * shard + (frame - lo_r) (orbfe_group_block_index; the unused slots of a slice are
 * zero) -- it extracts its shard straight into its own slice, and ONE in-place all-gather per block (ncclAllGather, RCCL)
 * leaves the whole batch on every rank.  The consumer of the gather, what KeyFrameDatabase /
 * LoopClosing do serially per candidate keyframe (src/LoopClosing.cc:312-342), is orbfe_group_match: frames of the own shard
 * against candidate frames anywhere in the gathered set.
 *
 * Two ways to form a group; every other call is the same:
 *   orbfe_group_create_local  ONE process drives ndevices devices (ncclCommInitAll): the shape of a C++ SLAM process
 *   orbfe_group_create_rank   one process per device: rank 0 makes an id (orbfe_group_unique_id), hands the 128 bytes to the
 *                             other ranks by any means it has, every rank calls this (ncclCommInitRank)
 * p->max_batch = the largest GLOBAL batch; p->device is ignored.  RCCL is loaded at run time (the copy already mapped into
 * the process if there is one, else librccl.so.1 / $ORBFE_RCCL_LIB); without it the create calls fail with ORBFE_ERR_STATE.
 * A group is used by one thread at a time.  Calls only enqueue work (compute stream + communication stream per member,
 * ordered by events); orbfe_group_synchronize / _get_frame / _match wait.
 *
 * Transport of the exchange step.  ORBFE_GROUP_RCCL (default): ncclAllGather.  ORBFE_GROUP_COPY (local groups only,
 * orbfe_group_create_local_ex): every member pulls the other members' slices with
 * hipMemcpyAsync / hipMemcpyPeerAsync on its communication stream behind the same events -- same bytes at the same offsets.
 * It needs no communicator, so `devices` may name one device several times: several members on ONE GPU, which is how the
 * multi-member paths are tested on a one-GPU box (RCCL refuses two ranks on one device).
 * ------------------------------------------------------------------------------------------- */
typedef struct orbfe_group orbfe_group;
enum { ORBFE_GROUP_RCCL = 0, ORBFE_GROUP_COPY = 1 };
void orbfe_group_shard_range(int32_t nframes, int32_t rank, int32_t world, int32_t *lo, int32_t *hi);
/* pure index arithmetic of the layout above (no group, no device): the rank that owns `frame`, and the frame's slot in the
 * blocks of a group with `shard` slots per rank; -1 on a bad argument */
int32_t orbfe_group_owner_rank(int32_t nframes, int32_t world, int32_t frame);
int32_t orbfe_group_block_index_of(int32_t nframes, int32_t world, int32_t shard, int32_t frame);
orbfe_status orbfe_group_unique_id(uint8_t id[128]);
orbfe_status orbfe_group_create_local(const orbfe_params *p, const int32_t *devices, int32_t ndevices, orbfe_group **out);
orbfe_status orbfe_group_create_local_ex(const orbfe_params *p, const int32_t *devices, int32_t ndevices, int32_t transport,
                                         orbfe_group **out);
orbfe_status orbfe_group_create_rank(const orbfe_params *p, int32_t device, int32_t rank, int32_t world, const uint8_t id[128],
                                     orbfe_group **out);
void orbfe_group_destroy(orbfe_group *g);
int32_t orbfe_group_world(const orbfe_group *g);
int32_t orbfe_group_members(const orbfe_group *g);       /* members THIS process drives (world for a local group, 1 for a rank group) */
int32_t orbfe_group_transport(const orbfe_group *g);
int32_t orbfe_group_capacity(const orbfe_group *g);      /* cap: keypoint slots per frame of the blocks */
int32_t orbfe_group_frames_padded(const orbfe_group *g); /* F = world * shard */
int32_t orbfe_group_block_index(const orbfe_group *g, int32_t nframes, int32_t frame);
/* HOST frames of the global batch (grays[i] = frame i, w x ht, row pitch stride): every member of this process copies and
 * extracts its own shard (a rank group reads only grays[lo .. hi) of its rank) */
orbfe_status orbfe_group_extract_batch(orbfe_group *g, const uint8_t *const *grays, int32_t nframes, int32_t w, int32_t ht,
                                       int32_t stride);
/* DEVICE frames: d_gray = the shard of member `member` (its frames only, on its device), nframes_global = the size of the
 * whole batch (the shard bounds follow from it) */
orbfe_status orbfe_group_extract_shard_device(orbfe_group *g, int32_t member, const uint8_t *d_gray, int32_t nframes_global, int32_t w,
                                              int32_t ht, int32_t stride, size_t frame_stride);
/* the one exchange step: in-place ncclAllGather of the three blocks on the members' communication streams, behind the
 * extraction; later calls on the compute streams are ordered behind it */
orbfe_status orbfe_group_allgather(orbfe_group *g);
orbfe_status orbfe_group_synchronize(orbfe_group *g);
/* device pointers of member `member`'s blocks and its compute stream (hipStream_t), for consumers of the gathered batch */
orbfe_status orbfe_group_blocks(orbfe_group *g, int32_t member, int32_t **d_n, orbfe_keypoint **d_kps, uint8_t **d_desc,
                                void **compute_stream);
/* one frame of the (gathered) batch of the last extract call to the host */
orbfe_status orbfe_group_get_frame(orbfe_group *g, int32_t frame, orbfe_keypoint *kps, uint8_t *desc, int32_t cap, int32_t *n_out);
/* the same out of the blocks of member `member` (orbfe_group_get_frame reads member 0) */
orbfe_status orbfe_group_get_frame_from(orbfe_group *g, int32_t member, int32_t frame, orbfe_keypoint *kps, uint8_t *desc, int32_t cap,
                                        int32_t *n_out);
/* the whole count block [F] of member `member` to the host (slots outside the shards' frames are 0) */
orbfe_status orbfe_group_get_counts(orbfe_group *g, int32_t member, int32_t *n_out);
/* pair p: brute-force match (as orbfe_match_bf: best <= th, ratio, rotation histogram) of frame qframe[p] -- a frame of a
 * shard of THIS process -- against frame tframe[p], any frame of the batch; match [npairs][cap] (train index or -1, slots
 * >= the query frame's count are -1), nmatches [npairs].  HOST arrays; call after orbfe_group_allgather. */
orbfe_status orbfe_group_match(orbfe_group *g, const int32_t *qframe, const int32_t *tframe, int32_t npairs, float nnratio, int32_t th,
                               int32_t check_ori, int32_t *match, int32_t *nmatches);
/* the same on one member with everything on its device: pairs as BLOCK indices (orbfe_group_block_index), results
 * [npairs][cap] / [npairs] in device memory, enqueued on the member's compute stream */
orbfe_status orbfe_group_match_device(orbfe_group *g, int32_t member, const int32_t *d_qblock, const int32_t *d_tblock, int32_t npairs,
                                      float nnratio, int32_t th, int32_t check_ori, int32_t *d_match, int32_t *d_nmatches);

/* ---------------------------------------------------------------------------------------------
 * Formats: the on-disk keyframe records of Map::Save / Map::Load and the ORB vocabulary files
 * ------------------------------------------------------------------------------------------- */
/* Keyframe block of Map::Save (perfect/src/Map.cc:330-381 _WriteKeyFrame, read back by _ReadKeyFrame :143-187):
 *   u64 mnId | f64 mTimeStamp | f32 t_cw[3] | f32 q_cw[4] (x y z w) | i32 N |
 *   N x { f32 pt.x pt.y size angle response | i32 octave | u8 descriptor[32] | u64 map-point index (ULONG_MAX = none) }
 * = 48 + 64 * N bytes; class_id is not stored (the reader leaves -1).  HOST buffers; *written / *consumed = block size. */
size_t orbfe_mapio_keyframe_bytes(int32_t n);
orbfe_status orbfe_mapio_write_keyframe(uint8_t *dst, size_t cap, uint64_t id, double timestamp, const float t_cw[3],
                                        const float q_cw[4], const orbfe_keypoint *kps, const uint8_t *desc,
                                        const uint64_t *mp_index /* NULL = none */, int32_t n, size_t *written);
orbfe_status orbfe_mapio_read_keyframe(const uint8_t *src, size_t len, uint64_t *id, double *timestamp, float t_cw[3],
                                       float q_cw[4], orbfe_keypoint *kps, uint8_t *desc, uint64_t *mp_index, int32_t cap,
                                       int32_t *n, size_t *consumed);
/* the 64-byte feature records straight from an extractor output block in HBM (also what an all-gathered block is turned
 * into before it is written): frame b -> d_out + b*cap*64, slots >= d_n[b] zero; d_mp_index [nframes][cap] or NULL */
orbfe_status orbfe_mapio_pack_records_device(const orbfe_keypoint *d_kps, const uint8_t *d_desc, const int32_t *d_n,
                                             const uint64_t *d_mp_index, int32_t nframes, int32_t cap, uint8_t *d_out,
                                             void *stream);

/* The caller's colour -> gray step before operator() (Tracking::GrabImageRGBD, src/Tracking.cc:339-353) for DEVICE-resident
 * 3-channel interleaved frames: gray = (w0*c0 + 9617*c1 + w2*c2 + 8192) >> 14, (w0, w2) = (4899, 1868) when rgb_flag != 0
 * (cvtColor(CV_RGB2GRAY) on the memory order given -- the reference's path for cv::imread's BGR with Camera.RGB = 1),
 * (1868, 4899) otherwise (CV_BGR2GRAY).  Enqueued on `stream`. */
orbfe_status orbfe_interleaved_to_gray_device(const uint8_t *d_src, int32_t nframes, int32_t w, int32_t h, int32_t src_stride,
                                              size_t src_frame_stride, int32_t rgb_flag, uint8_t *d_gray,
                                              int32_t gray_stride, size_t gray_frame_stride, void *stream);

/* ORB vocabulary files as the reference loads them (src/System.cc:123-129; tool/text2binary.cc converts one into the
 * other).  DBoW2 is not vendored by the reference; the two layouts are ORB-SLAM2's TemplatedVocabulary
 * loadFromTextFile / saveToBinaryFile, restated (csrc/orbfe_io.hip).  Host only: no device is touched before
 * orbfe_vocabulary_create_from_file. */
typedef struct orbfe_vocfile orbfe_vocfile;
orbfe_status orbfe_vocfile_load(const char *path /* ORBvoc.txt or ORBvoc.bin */, orbfe_vocfile **out);
void orbfe_vocfile_free(orbfe_vocfile *v);
orbfe_status orbfe_vocfile_info(const orbfe_vocfile *v, int32_t *k, int32_t *L, int32_t *nnodes, int32_t *nwords,
                                int32_t *scoring, int32_t *weighting);
/* pointers into the parsed file (valid until orbfe_vocfile_free); any may be NULL */
orbfe_status orbfe_vocfile_arrays(const orbfe_vocfile *v, const uint32_t **child_off, const uint32_t **child_idx,
                                  const uint8_t **node_desc, const uint32_t **word_id, const double **weight,
                                  const uint32_t **parent, const uint8_t **is_leaf);
orbfe_status orbfe_vocfile_save_binary(const orbfe_vocfile *v, const char *path);
/* orbfe_vocabulary_create on the parsed tree; a file that holds the header only gives the empty vocabulary described there */
orbfe_status orbfe_vocabulary_create_from_file(int32_t device, const orbfe_vocfile *v, orbfe_vocabulary **out);

/* ---- the fork's optical-flow dynamic-point mask (csrc/orbfe_flow.hip, DESIGN.md "Optical-flow mask") ----------------------
 * FlowSLAM::Flow::ComputeMask(GrayImg, mask, th) (perfect/src/Flow.cc:15-52): th = max(th, 40); pyrDown to (w/2, h/2);
 * with a previous half-size frame, Farneback flow (0.5, 3, 15, 3, 5, 1.2, 0) from it to this one, pyrUp (not rescaled),
 * mask = 0 where fx*fx + fy*fy >= th, then erode, erode, dilate with the 21x21 ellipse; without one, all ones.  The state
 * becomes this frame's half-size image.  Bit-exact against tests/flow_oracle.py (an unpinned restatement of OpenCV 3.2).
 * Frames are at least 16 x 16 and at most max_width x max_height.  A frame whose half size differs from the stored
 * previous frame's returns ORBFE_ERR_SIZE and leaves the state unchanged (OpenCV would throw). */
typedef struct orbfe_flow orbfe_flow;   /* one FlowSLAM::Flow: device scratch, own stream, the previous half-size frame */
orbfe_status orbfe_flow_create(int32_t device, int32_t max_width, int32_t max_height, int32_t max_batch, orbfe_flow **out);
void orbfe_flow_destroy(orbfe_flow *f);
orbfe_status orbfe_flow_reset(orbfe_flow *f);            /* forget the previous frame (mImGrayLast empty) */
void *orbfe_flow_get_stream(orbfe_flow *f);
/* one HOST frame in, HOST mask out (w x h, row pitch mask_stride), state advanced; synchronous */
orbfe_status orbfe_flow_compute_mask(orbfe_flow *f, const uint8_t *gray, int32_t w, int32_t h, int32_t stride, float threshold,
                                     uint8_t *mask, int32_t mask_stride);
/* Sequence form, DEVICE buffers: mask i comes from (frame i-1, frame i); mask 0 from the previous call's last frame, or all ones
 * when there is none.  d_mask_ones[i] = sum of mask i (may be NULL).  At most max_batch frames.  Enqueued on `stream`
 * (NULL = HIP's default stream), no synchronisation; the handle's scratch is reused by the next call on any stream. */
orbfe_status orbfe_flow_compute_masks_device(orbfe_flow *f, const uint8_t *d_gray, int32_t nframes, int32_t w, int32_t h,
                                             int32_t stride, size_t frame_stride, float threshold, uint8_t *d_mask,
                                             int32_t mask_stride, size_t mask_frame_stride, int32_t *d_mask_ones, void *stream);
/* ComputeMask(GrayImg, Homo, mask, th) (perfect/src/Flow.cc:73-80): warpPerspective(GrayImg, dest, Homo, GrayImg.size()) as
 * OpenCV 3.2 computes it (INTER_LINEAR, BORDER_CONSTANT 0: M inverted by invert(DECOMP_LU), all zeros when singular; the
 * invoker's 64-column blocks; 1/32-pixel fixed-point bilinear remap), then the plain ComputeMask on the warped frame.  homo: 9
 * doubles, row-major, as findHomography returns it (NOT inverted).  The state becomes the WARPED frame's half-size image, so
 * the next pair compares two warped frames (the reference's behaviour, kept).  Host frame in, host mask out, synchronous.
 * A NULL homo returns ORBFE_ERR_ARG; size and state rules as orbfe_flow_compute_mask. */
orbfe_status orbfe_flow_compute_mask_homo(orbfe_flow *f, const uint8_t *gray, int32_t w, int32_t h, int32_t stride,
                                          const double *homo, float threshold, uint8_t *mask, int32_t mask_stride);
/* Sequence form.  d_homo: DEVICE [nframes][9] doubles; d_use_homo: DEVICE int32 [nframes], frame i is warped iff nonzero
 * (NULL = every frame), so a replay can mix tracked and lost frames as TrackHomo does.  Otherwise as
 * orbfe_flow_compute_masks_device: enqueued on `stream`, no synchronisation, passes of at most 64 frames, state carried. */
orbfe_status orbfe_flow_compute_masks_homo_device(orbfe_flow *f, const uint8_t *d_gray, int32_t nframes, int32_t w, int32_t h,
                                                  int32_t stride, size_t frame_stride, const double *d_homo,
                                                  const int32_t *d_use_homo, float threshold, uint8_t *d_mask,
                                                  int32_t mask_stride, size_t mask_frame_stride, int32_t *d_mask_ones,
                                                  void *stream);
/* perfect/src/Frame.cc:360-377 on the padded device blocks of orbfe_extract_batch_device, in place: frame i keeps only the
 * keypoints with mask[(int)y][(int)x] == 1 when d_mask_ones[i] > w*h*0.65, in order, descriptors following; slots >= the new
 * d_n[i] are zero-filled again (the all-gather invariant).  Enqueued on `stream`.
 * d_mask_ones[i] is the SUM of mask i's values (cv::sum), as orbfe_flow_compute_masks*_device write it; for a 0 / 1 mask, its
 * count of ones.  A mask value other than 1 under a keypoint drops it.  The reference reads the plane unchecked; here a
 * keypoint is in the plane iff x > -1 && x < w && y > -1 && y < h, decided in float before the truncation (so a NaN or an
 * infinity is out, and (-1, 0) truncates to column / row 0), and a keypoint outside the plane is dropped.  d_n[i] > cap
 * counts as cap. */
orbfe_status orbfe_mask_keypoints_device(const uint8_t *d_mask, int32_t w, int32_t h, int32_t mask_stride, size_t mask_frame_stride,
                                         const int32_t *d_mask_ones, int32_t nframes, orbfe_keypoint *d_kps, uint8_t *d_desc,
                                         int32_t *d_n, int32_t cap, void *stream);
/* Test taps of the last compute call (synchronises the handle's last stream).  `frame` counts in that call, among its last
 * min(max_batch, 64) frames.  stage / what / dst layout (w, h receive the size):
 *   0 ORBFE_FLOW_TAP_HALF    the half-size frame                           uint8  [h][w]
 *   1 ORBFE_FLOW_TAP_FLOW    flow of pyramid level `level` (0 = finest)    float  [h][w][2]
 *   2 ORBFE_FLOW_TAP_FLOW2   the pyrUp'ed flow                             float  [h][w][2]
 *   3 ORBFE_FLOW_TAP_PRE     the thresholded mask before morphology       uint8  [h][w]
 *   4 ORBFE_FLOW_TAP_MASK    the final mask                                uint8  [h][w]
 *   5 ORBFE_FLOW_TAP_POLY    PolyExp of the frame at `level`               float  [h][w][5]
 *   6 ORBFE_FLOW_TAP_WARP    the warped full-size frame pyrDown read        uint8  [h][w]
 * Stages 1-3 of a frame that had no previous frame return ORBFE_ERR_STATE, and so does stage 6 of a frame that was not warped. */
enum { ORBFE_FLOW_TAP_HALF = 0, ORBFE_FLOW_TAP_FLOW = 1, ORBFE_FLOW_TAP_FLOW2 = 2, ORBFE_FLOW_TAP_PRE = 3, ORBFE_FLOW_TAP_MASK = 4,
       ORBFE_FLOW_TAP_POLY = 5, ORBFE_FLOW_TAP_WARP = 6 };
orbfe_status orbfe_flow_tap(orbfe_flow *f, int32_t frame, int32_t stage, int32_t level, void *dst, size_t cap, int32_t *w, int32_t *h);
/* Host-side constants, no device needed: the level plan of a w x h frame's half-size image (level 0 = finest; lw, lh, ksize
 * [4], taps [4][19]: the GaussianBlur taps of each level) and FarnebackPrepareGaussian's g, xg, xxg ([3][11], x = -5..5)
 * and ig11, ig03, ig33, ig55. */
orbfe_status orbfe_flow_plan(int32_t w, int32_t h, int32_t *nlevels, int32_t *lw, int32_t *lh, int32_t *ksize, float *taps);
orbfe_status orbfe_flow_poly_constants(float *g, double *ig);

/* ---- the fork's homography estimate (csrc/orbfe_homography.hip) ---------------------------------------
 * cv::findHomography(src, dst, method, threshold, mask, max_iters, confidence) of OpenCV 3.2 for method RANSAC (8) and 0 (least
 * squares over all points), as Tracking::TrackHomo (perfect/src/Tracking.cc:1331-1399) calls it: src = points_current,
 * dst = points_last, dst ~ H * src.  RANSAC: RNG((uint64)-1), getSubset, runKernel (normalised DLT, JacobiImpl_ eigen),
 * float computeError, acceptance goodCount > max(maxGoodCount, 3), RANSACUpdateNumIters; then (n > 4) the refit over the
 * inliers and the 10-iteration Levenberg-Marquardt refinement.  Bit-exact against tests/homography_oracle.py (an unpinned
 * restatement).  Points are (x, y) float pairs.  threshold <= 0 means 3.  Output H: 9 doubles, row-major (H22 from runKernel's
 * 1./H22 scaling), all zeros with ok = 0 when there is no model (n < 4, no subset, no model with more than 3 inliers, a failed
 * method-0 fit); the mask (1 = inlier) is then all zeros.  An unknown method, a RANSAC confidence outside (0, 1), n > max_pairs
 * or nsets > max_sets return ORBFE_ERR_ARG. */
#define ORBFE_HOMOGRAPHY_RANSAC 8
typedef struct orbfe_homography orbfe_homography;   /* device scratch for one host call, test taps, own stream */
orbfe_status orbfe_homography_create(int32_t device, int32_t max_pairs, int32_t max_sets, orbfe_homography **out);
void orbfe_homography_destroy(orbfe_homography *h);
void *orbfe_homography_get_stream(orbfe_homography *h);
/* HOST points in, HOST H / mask out, synchronous.  mask (n bytes) may be NULL.  *ok = the result (!H.empty()). */
orbfe_status orbfe_find_homography(orbfe_homography *h, const float *src_xy, const float *dst_xy, int32_t n, int32_t method,
                                   double threshold, int32_t max_iters, double confidence, double *H, uint8_t *mask, int32_t *ok);
/* Batched form, DEVICE buffers: set i holds pairs [d_offsets[i], d_offsets[i+1]) of d_src_xy / d_dst_xy (CSR); its mask goes to
 * the same range of d_mask (required).  d_H [nsets][9], d_ok [nsets]: ok = result && n_i > min_pairs, so min_pairs = 50 gives
 * TrackHomo's `points_current.size() > 50 && !homo.empty()`, and (d_H, d_ok) are exactly the (d_homo, d_use_homo) of
 * orbfe_flow_compute_masks_homo_device.  A set with n_i > max_pairs gets ok = 0 and a zero H; its mask is not written.
 * Enqueued on `stream` (NULL = HIP's default stream), no synchronisation; the taps of the handle are overwritten. */
orbfe_status orbfe_find_homographies_device(orbfe_homography *h, const int32_t *d_offsets, const float *d_src_xy,
                                            const float *d_dst_xy, int32_t nsets, int32_t method, double threshold,
                                            int32_t max_iters, double confidence, int32_t min_pairs, double *d_H, int32_t *d_ok,
                                            uint8_t *d_mask, void *stream);
/* Test taps of set `set` of the last call (synchronises the handle's last stream):
 *   0 ORBFE_HOMO_TAP_RANSAC  the best RANSAC model (zeros unless RANSAC found one)                       double [9]
 *   1 ORBFE_HOMO_TAP_INFO    RANSAC result, iterations run (the loop counter at exit), final niters,
 *                            refit accepted (runKernel over the inliers succeeded)                        int32 [4]
 *   2 ORBFE_HOMO_TAP_REFIT   the refit model before Levenberg-Marquardt (zeros when not refitted)         double [9]
 * The RANSAC mask is the call's mask output.  ORBFE_ERR_STATE for a set the last call did not have. */
enum { ORBFE_HOMO_TAP_RANSAC = 0, ORBFE_HOMO_TAP_INFO = 1, ORBFE_HOMO_TAP_REFIT = 2 };
orbfe_status orbfe_homography_tap(orbfe_homography *h, int32_t set, int32_t stage, void *dst, size_t cap);
/* Known-answer runs of the device primitives on HOST arrays (synchronous, current device):
 *   0 ORBFE_HOMO_KAT_RNG       in: uint64 initial state; out: n uint32 of cv::RNG::next()
 *   1 ORBFE_HOMO_KAT_HYPOT     in: n (a, b) doubles; out: n doubles of lapack.cpp's hypot
 *   2 ORBFE_HOMO_KAT_NUMITERS  in: n (p, ep, max_iters) doubles; out: n int32 RANSACUpdateNumIters(p, ep, 4, max_iters)
 *   3 ORBFE_HOMO_KAT_JACOBI9   in: n 9x9 doubles; out: n x (9 eigenvalues, 9x9 eigenvector rows) of JacobiImpl_
 *   4 ORBFE_HOMO_KAT_JACOBI8   in: n 8x8 doubles; out: n x (8, 8x8) */
enum { ORBFE_HOMO_KAT_RNG = 0, ORBFE_HOMO_KAT_HYPOT = 1, ORBFE_HOMO_KAT_NUMITERS = 2, ORBFE_HOMO_KAT_JACOBI9 = 3,
       ORBFE_HOMO_KAT_JACOBI8 = 4 };
orbfe_status orbfe_homography_kat(int32_t what, int32_t n, const void *in, void *out);

/* ---- the per-frame geometry of the RGB-D Frame (csrc/orbfe_frame.hip) ----------------------------------
 * cv::undistortPoints(src, dst, K, D, noArray(), P) of OpenCV 3.2 (cvUndistortPoints: double arithmetic, 5 fixed iterations when
 * there are coefficients), Frame::UndistortKeyPoints (perfect/src/Frame.cc:750-781), Frame::ComputeImageBounds (:784-815),
 * Frame::ComputeStereoFromRGBD (:1041-1062) and Tracking's depth convertTo (perfect/src/Tracking.cc:681-682).  One __host__
 * __device__ function (csrc/orbfe_undistort.h) serves the kernels and the host bounds helper.  Bit-exact against
 * tests/undistort_oracle.py (an unpinned restatement).  The tilted model (14 coefficients) and a rectification R are not built. */
typedef struct orbfe_camera {
    float K[9];       /* mK, row-major 3x3 (CV_32F): fx = K[0], cx = K[2], fy = K[4], cy = K[5]; the skew K[1] is not read */
    float P[9];       /* new camera matrix of undistortPoints (row-major 3x3), read when has_P != 0; the Frame passes P = K */
    int32_t has_P;    /* 0: P absent -- identity, the results are normalised coordinates */
    float dist[12];   /* mDistCoef: k1 k2 p1 p2 [k3 [k4 k5 k6 [s1 s2 s3 s4]]] */
    int32_t ndist;    /* 0, 4, 5, 8 or 12 (ORB-SLAM passes 4, or 5 when k3 != 0: perfect/src/Tracking.cc:154-165); else ORBFE_ERR_ARG */
    float bf;         /* mbf = baseline * fx (uRight = x_un - bf / depth) */
} orbfe_camera;
#define ORBFE_DEPTH_U16 0 /* depth plane of uint16: d = (float)u * scale (convertTo(CV_32F, scale)) */
#define ORBFE_DEPTH_F32 1 /* depth plane of float: d = v * scale when fabs(scale - 1.0f) > 1e-5 (Tracking's condition), else v */
/* cv::undistortPoints on n HOST points (x, y) float pairs -> out_xy (may alias xy), on the matcher's stream, synchronous.  No k1
 * shortcut: every point goes through the iterations (what the Frame skips when k1 == 0 is the caller's business). */
orbfe_status orbfe_undistort_points(orbfe_matcher *m, const float *xy, int32_t n, const orbfe_camera *cam, float *out_xy);
/* Frame::ComputeImageBounds(imLeft) for a w x ht image, host only: out = {minX, maxX, minY, maxY, gw_inv, gh_inv}.  dist[0] == 0
 * (or ndist == 0): {0, w, 0, ht}; else the corners (0, 0), (w, 0), (0, ht), (w, ht) undistorted as orbfe_undistort_points does
 * (with cam's P) and minX = min(x0, x2), maxX = max(x1, x3), minY = min(y0, y1), maxY = max(y2, y3).  gw_inv = 64.f / (maxX - minX)
 * and gh_inv = 48.f / (maxY - minY) in float (src/Frame.cc:401-402): the arguments orbfe_assign_grid* take. */
orbfe_status orbfe_image_bounds(const orbfe_camera *cam, int32_t w, int32_t ht, float out[6]);
/* UndistortKeyPoints + ComputeStereoFromRGBD for every frame of an extractor output block (d_kps [nframes][cap], d_n [nframes]
 * as orbfe_extract_batch_device or orbfe_mask_keypoints_device left them), device-resident:
 *   d_kps_un [nframes][cap]   mvKeysUn: a copy of the keypoint with x, y undistorted; dist[0] == 0 (or ndist == 0): the copy is
 *                             untouched -- the reference's k1-only test (Frame.cc:752), so k1 = 0 with k2 != 0 is NOT undistorted
 *   d_depth / d_uright [nframes][cap]   mvDepth / mvuRight: d = the depth plane at ((int)y, (int)x) of the DISTORTED keypoint;
 *                             d > 0: depth = d, uRight = x_un - bf / d (float), else -1 / -1.  A keypoint outside the plane has no
 *                             depth (-1 / -1; undefined in the reference).  d_depth_plane == NULL (monocular and stereo Frames):
 *                             -1 / -1 for all.  d_depth / d_uright may be NULL together (keypoints only).
 * Slots >= d_n[f] of all three outputs are zero-filled (the all-gather invariant).  The depth plane of frame f starts at
 * d_depth_plane + f * depth_frame_stride, rows depth_stride bytes apart, depth_w x depth_h elements of depth_format
 * (ORBFE_DEPTH_*); scale = the float 1.0f / DepthMapFactor.  Enqueued on `stream`, no synchronisation. */
orbfe_status orbfe_frame_geometry_batch_device(orbfe_matcher *m, const orbfe_keypoint *d_kps, const int32_t *d_n, int32_t cap,
                                               int32_t nframes, const orbfe_camera *cam, const void *d_depth_plane, int32_t depth_w,
                                               int32_t depth_h, int32_t depth_format, size_t depth_stride, size_t depth_frame_stride,
                                               float scale, orbfe_keypoint *d_kps_un, float *d_depth, float *d_uright, void *stream);
/* mImDepth.convertTo(mImDepth, CV_32F, scale) for nframes w x ht planes (Tracking.cc:681-682), DEVICE buffers: u16 planes always,
 * f32 planes scaled under Tracking's condition (else copied); dst = (float)src * scale + 0.0f, as cvtScale_ computes it.  Strides
 * in bytes.  Enqueued on `stream`, no synchronisation. */
orbfe_status orbfe_depth_to_float_device(const void *d_src, int32_t depth_format, int32_t nframes, int32_t w, int32_t ht,
                                         size_t src_stride, size_t src_frame_stride, float scale, float *d_dst, size_t dst_stride,
                                         size_t dst_frame_stride, void *stream);

/* ---- Sim3Solver's RANSAC (csrc/orbfe_sim3.hip) ----------------------------------------------------------
 * The reference's Sim3Solver (src/Sim3Solver.cc): Horn's closed form on three correspondences inside the RANSAC loop of
 * `iterate`, the step of LoopClosing::ComputeSim3 between SearchByBoW and SearchBySim3.  The inputs are the constructor's
 * quantities of the N correspondences: camera-frame points X1[i] = Rcw1 * Xw1 + tcw1 and X2[i] (orbfe_sim3_prepare_device
 * computes them), the two level sigma^2 values (the threshold is (size_t)(9.210 * sigma2), truncated as in the reference) and
 * the two cameras as K = (fx, fy, cx, cy).  The random draws are an INPUT: 3 * n_iterations raw values r in [0, 2^31 - 1] (bit 31
 * is ignored), each used as DUtils' RandomInt(0, size - 1) = (int)(((double)r / 2147483648.0) * size); with r = rand() the
 * stream is the reference's.  A call consumes three draws per iteration it ran (result.iterations_run); a caller that wants the
 * reference's exact stream keeps the rest.  Bit-exact against the canonical mode of tests/sim3_oracle.py (an unpinned
 * restatement); atan2 / sin / cos are fixed fp64 operation sequences, not a C library's. */
typedef struct orbfe_sim3_model {
    float T12[16];     /* row-major 4x4 [s*R t; 0 0 0 1] */
    float R[9];        /* GetEstimatedRotation */
    float t[3];        /* GetEstimatedTranslation */
    float s;           /* GetEstimatedScale */
    float reserved[3];
} orbfe_sim3_model;
typedef struct orbfe_sim3_state {   /* what a solver carries from one iterate call to the next; all zero = a new solver */
    int32_t iterations;             /* mnIterations (SetRansacParameters sets it to 0) */
    int32_t best_inliers;           /* mnBestInliers */
    int32_t reserved[2];
    orbfe_sim3_model best;          /* mBestT12 / mBestRotation / mBestTranslation / mBestScale */
} orbfe_sim3_state;
typedef struct orbfe_sim3_result {
    int32_t found;                  /* iterate returned a model: n_inliers > min_inliers at an iteration whose count reached the best */
    int32_t no_more;                /* bNoMore */
    int32_t n_inliers;              /* nInliers (0 unless found) */
    int32_t iterations_run;         /* iterations of this call */
    orbfe_sim3_model model;         /* T12: the returned matrix, all zeros unless found; R, t, s: the getters (the best so far) */
} orbfe_sim3_result;
typedef struct orbfe_sim3_set {     /* one set of the batched form */
    float K1[4], K2[4];             /* fx, fy, cx, cy of keyframe 1 and 2 */
    int32_t fix_scale;              /* mbFixScale: scale 1 (stereo / RGB-D) */
    int32_t min_inliers;            /* mRansacMinInliers */
    int32_t max_its;                /* mRansacMaxIts, already clamped (orbfe_sim3_ransac_iterations) */
    int32_t n_iterations;           /* iterate's nIterations */
    int32_t draws_offset;           /* the set's 3 * n_iterations draws start here in d_draws */
    int32_t key_offset, n_keys;     /* the set's slice of d_key_mask: mN1 bytes (d_idx1 form) */
    int32_t reserved;
} orbfe_sim3_set;
typedef struct orbfe_sim3_iter {    /* tap record of one iteration run */
    int32_t triple[3];
    int32_t n_inliers;
    float T12[16];
} orbfe_sim3_iter;
typedef struct orbfe_sim3 orbfe_sim3;   /* device scratch for one host call, test taps, own stream */
orbfe_status orbfe_sim3_create(int32_t device, int32_t max_pairs, int32_t max_sets, orbfe_sim3 **out);
void orbfe_sim3_destroy(orbfe_sim3 *h);
void *orbfe_sim3_get_stream(orbfe_sim3 *h);
/* SetRansacParameters' iteration clamp, host only (the host's libm): 1 when min_inliers == n, else
 * ceil(log(1 - p) / log(1 - pow((float)min_inliers / n, 3))), then max(1, min(that, max_its)).  1 for n < min_inliers. */
int32_t orbfe_sim3_ransac_iterations(double probability, int32_t min_inliers, int32_t max_its, int32_t n);
/* One solver's iterate(n_iterations): HOST arrays in and out, synchronous.  X1 / X2 [n][3], sigma2_1 / sigma2_2 [n], draws
 * [3 * n_iterations].  state and best_mask [n] (mvbBestInliers) are in / out: zeroed they are a new solver.  mask [n] (may be NULL):
 * the inliers over the n correspondences when found, else zeros.  n < min_inliers (or n < 3, undefined in the reference): no
 * model, no_more = 1.  n > max_pairs, n_iterations < 0 or past 2^20, negative counters: ORBFE_ERR_ARG, nothing is launched. */
orbfe_status orbfe_sim3_iterate(orbfe_sim3 *h, const float *X1, const float *X2, const float *sigma2_1, const float *sigma2_2,
                                int32_t n, const float *K1, const float *K2, int32_t fix_scale, int32_t min_inliers, int32_t max_its,
                                int32_t n_iterations, const int32_t *draws, orbfe_sim3_state *state, uint8_t *best_mask,
                                orbfe_sim3_result *result, uint8_t *mask);
/* Batched form, DEVICE buffers: the solvers of one ComputeSim3 round in one launch.  Set i holds correspondences [d_offsets[i],
 * d_offsets[i+1]) of d_X1 / d_X2 / d_sigma2_* (CSR); its masks go to the same range of d_best_mask (in / out) and d_mask; its
 * parameters are d_sets[i], its state d_state[i] (in / out), its result d_result[i].  A set with n_i > max_pairs gets found = 0,
 * no_more = 1, n_inliers = 0 and iterations_run = 0 in d_result[i] and nothing else of it is written (state, masks, model).
 * d_idx1 (optional, together with d_key_mask; CSR like the points): mvnIndices1, the keypoint index in keyframe 1 of every
 * correspondence.  The set's n_keys bytes of d_key_mask at key_offset are then iterate's vbInliers: zeroed, and on a return
 * d_key_mask[key_offset + d_idx1[j]] = 1 for every inlier j (an index outside [0, n_keys) is skipped), which lines up with the
 * vpMatched12 SearchBySim3 takes.  Enqueued on `stream` (NULL = HIP's default stream), no synchronisation; the handle's taps
 * are overwritten. */
orbfe_status orbfe_sim3_iterate_device(orbfe_sim3 *h, const int32_t *d_offsets, const float *d_X1, const float *d_X2,
                                       const float *d_sigma2_1, const float *d_sigma2_2, const orbfe_sim3_set *d_sets,
                                       const int32_t *d_draws, int32_t nsets, orbfe_sim3_state *d_state, uint8_t *d_best_mask,
                                       orbfe_sim3_result *d_result, uint8_t *d_mask, const int32_t *d_idx1, uint8_t *d_key_mask,
                                       void *stream);
/* The constructor's mvX3Dc1 / mvX3Dc2 on DEVICE buffers: d_X1[i] = Rcw1 * d_world1[i] + tcw1 and likewise for keyframe 2, n map
 * point pairs; the poses are HOST arrays (row-major 3x3, 3).  Enqueued on `stream`, no synchronisation. */
orbfe_status orbfe_sim3_prepare_device(orbfe_sim3 *h, const float *d_world1, const float *d_world2, int32_t n, const float *Rcw1,
                                       const float *tcw1, const float *Rcw2, const float *tcw2, float *d_X1, float *d_X2, void *stream);
/* Test taps of set `set` of the last call (synchronises the handle's last stream).  A handle holds and writes no taps until
 * orbfe_sim3_set_tap_iteration is first called on it (that call allocates them; ORBFE_ERR_NOMEM if it cannot); from then on every
 * call records them for its first ORBFE_SIM3_TAP_SETS sets:
 *   0 ORBFE_SIM3_TAP_ITERATIONS  one orbfe_sim3_iter per iteration run (the first ORBFE_SIM3_TAP_ITERS of them); *count = records
 *   1 ORBFE_SIM3_TAP_ERRORS      err1 / err2 of CheckInliers, float [n][2], of the iteration (counted within the call) chosen
 *                                with orbfe_sim3_set_tap_iteration BEFORE the call (default 0); *count = n.  ORBFE_ERR_STATE
 *                                when the call did not run that iteration.
 * ORBFE_ERR_STATE for a set the taps of the last call do not cover (every set, on a handle whose taps were never asked for). */
#define ORBFE_SIM3_TAP_SETS 32
#define ORBFE_SIM3_TAP_ITERS 512
enum { ORBFE_SIM3_TAP_ITERATIONS = 0, ORBFE_SIM3_TAP_ERRORS = 1 };
orbfe_status orbfe_sim3_set_tap_iteration(orbfe_sim3 *h, int32_t iteration);
orbfe_status orbfe_sim3_tap(orbfe_sim3 *h, int32_t set, int32_t stage, void *dst, size_t cap, int32_t *count);
/* Known-answer runs of the device primitives on HOST arrays (synchronous, current device):
 *   0 ORBFE_SIM3_KAT_JACOBI4   in: n 4x4 floats; out: n x (4 eigenvalues, 4x4 eigenvector rows) of JacobiImpl_<float>
 *   1 ORBFE_SIM3_KAT_ATAN2     in: n (y, x) doubles; out: n doubles of the canonical atan2
 *   2 ORBFE_SIM3_KAT_SIN       in: n doubles; out: n doubles of the canonical sin
 *   3 ORBFE_SIM3_KAT_COS       likewise, cos
 *   4 ORBFE_SIM3_KAT_ROTATION  in: n 4x4 float N matrices; out: n 3x3 float rotations (eigen, angle-axis, Rodrigues) */
enum { ORBFE_SIM3_KAT_JACOBI4 = 0, ORBFE_SIM3_KAT_ATAN2 = 1, ORBFE_SIM3_KAT_SIN = 2, ORBFE_SIM3_KAT_COS = 3, ORBFE_SIM3_KAT_ROTATION = 4 };
orbfe_status orbfe_sim3_kat(int32_t what, int32_t n, const void *in, void *out);

/* ---- The fork's dense point-cloud map (csrc/orbfe_cloud.hip) ---------------------------------------------
 * PointCloudMapping::viewer() of the reference (src/pointcloudmapping.cc) without the detector and the viewer (the outlier filter
 * and the cluster database follow in the next section): draw_rect_with_depth_threshold, generatePointCloud + pcl::transformPointCloud,
 * removeNaNFromPointCloud, the append to globalMap and pcl::VoxelGrid.  Bit-exact against tests/cloud_oracle.py (an unpinned
 * oracle: PCL is restated from knowledge, its assumptions are the list P1 .. P16 there).  Inside a voxel the points are summed in
 * ascending input position (a stable sort); std::sort leaves that order open.
 * A point is pcl::PointXYZRGBA without its padding: rgba = a << 24 | r << 16 | g << 8 | b.  Every record buffer is 16-byte
 * aligned.  Strides are in bytes.  The *_device calls take DEVICE buffers, run on `stream` and return after it has drained: each
 * of them reports sizes the host needs. */
typedef struct orbfe_cloud_point {
    float x, y, z;
    uint32_t rgba;
} orbfe_cloud_point;
typedef struct orbfe_cloud orbfe_cloud;
/* resolution: the voxel leaf (the float leaf is (float)resolution); max_points: records the map can hold, including the points of
 * an insert before its filter pass, and the most orbfe_cloud_voxel_filter_device takes; max_frames: keyframes of one generate /
 * insert call; w x ht: the keyframe size. */
orbfe_status orbfe_cloud_create(int32_t device, double resolution, int32_t max_points, int32_t max_frames, int32_t w, int32_t ht,
                                orbfe_cloud **out);
void orbfe_cloud_destroy(orbfe_cloud *h);
void *orbfe_cloud_get_stream(orbfe_cloud *h);
/* draw_rect_with_depth_threshold for the boxes of ONE frame, in list order (the caller has dropped the detections with
 * prob <= 0.54).  boxes [nboxes][4] = cv::Rect_<float> x, y, width, height and colors [nboxes][3] = the bytes stored at
 * color[3 j + 0 .. 2] are HOST arrays.  The colour plane is painted in place; the flat pixel indices of box b (ascending) follow
 * those of box b - 1 in d_indices, counts[b] (host) of them.  idx_cap < the sum of (height - 1) * (width - 2) over the boxes (the
 * most they can record): ORBFE_ERR_CAP, *n_out = that sum.  A box for which an index the reference would read or write lies
 * outside the plane (undefined there), whose numbers are not finite or reach 2^20, or whose painted width exceeds w:
 * ORBFE_ERR_ARG, nothing is written.  *n_out = indices recorded. */
orbfe_status orbfe_cloud_paint_boxes_device(orbfe_cloud *h, const float *d_depth, size_t depth_stride, uint8_t *d_bgr, size_t bgr_stride,
                                            const float *boxes, const uint8_t *colors, int32_t nboxes, int32_t *d_indices,
                                            int32_t idx_cap, int32_t *counts, int32_t *n_out, void *stream);
/* generatePointCloud, transformPointCloud and removeNaNFromPointCloud for nframes keyframes: float depth planes, BGR planes,
 * intrinsics [nframes][4] = fx, fy, cx, cy and T [nframes][16] = T.inverse().matrix() row-major in double (HOST arrays; see
 * orbfe_cloud_pose_matrix).  d_out receives the finite points of frame 0 in pixel order, then frame 1's, ...; counts[f] (host) and
 * *n_out tell how many.  More than cap: ORBFE_ERR_CAP, *n_out = the need, d_out untouched. */
orbfe_status orbfe_cloud_generate_device(orbfe_cloud *h, const float *d_depth, size_t depth_stride, size_t depth_frame_stride,
                                         const uint8_t *d_bgr, size_t bgr_stride, size_t bgr_frame_stride, int32_t nframes,
                                         const float *intrinsics, const double *T, orbfe_cloud_point *d_out, int32_t cap,
                                         int32_t *counts, int32_t *n_out, void *stream);
/* What viewer() does when it wakes up to nframes new keyframes: generate each, append to the map, then one VoxelGrid pass over
 * the map.  Map size + new points > max_points: ORBFE_ERR_CAP, *n_out = the need, the map unchanged.  *n_out = the map's size
 * after the call; *overflow = 1 when PCL's grid-size check (more than INT_MAX cells) left the map unfiltered. */
orbfe_status orbfe_cloud_insert_device(orbfe_cloud *h, const float *d_depth, size_t depth_stride, size_t depth_frame_stride,
                                       const uint8_t *d_bgr, size_t bgr_stride, size_t bgr_frame_stride, int32_t nframes,
                                       const float *intrinsics, const double *T, int32_t *counts, int32_t *n_out, int32_t *overflow,
                                       void *stream);
/* one keyframe from HOST planes (w floats / 3 w bytes per row, no padding), on the handle's stream */
orbfe_status orbfe_cloud_insert(orbfe_cloud *h, const float *depth, const uint8_t *bgr, const float *intrinsics, const double *T,
                                int32_t *n_out, int32_t *overflow);
/* pcl::VoxelGrid (the handle's leaf) over n <= max_points records; d_out (cap records) may not overlap d_in.  n = 0 or no finite
 * point: 0 voxels.  More than INT_MAX cells: ORBFE_OK, *overflow = 1 and the input copied through (cap < n: ORBFE_ERR_CAP).
 * More voxels than cap: ORBFE_ERR_CAP, *n_out = the need. */
orbfe_status orbfe_cloud_voxel_filter_device(orbfe_cloud *h, const orbfe_cloud_point *d_in, int32_t n, orbfe_cloud_point *d_out,
                                             int32_t cap, int32_t *n_out, int32_t *overflow, void *stream);
/* the map: its size, its records on the device (valid until the next insert / upload), a copy to the host (cap < size:
 * ORBFE_ERR_CAP, *n_out = size), and its replacement by n device records (n = 0 empties it) */
int32_t orbfe_cloud_size(const orbfe_cloud *h);
const orbfe_cloud_point *orbfe_cloud_data_device(const orbfe_cloud *h);
orbfe_status orbfe_cloud_download(orbfe_cloud *h, orbfe_cloud_point *dst, int32_t cap, int32_t *n_out);
orbfe_status orbfe_cloud_upload_device(orbfe_cloud *h, const orbfe_cloud_point *d_points, int32_t n, void *stream);
/* Host only: Converter::toSE3Quat(Tcw) followed by Isometry3d::inverse().matrix() -- the float pose widened to double, its
 * rotation through g2o's normalised quaternion and back, then R^T and -(R^T) t; row-major in and out.  Restated from knowledge of
 * Eigen 3.2 / g2o (oracle P15, P16); a caller that links Eigen passes its own matrix to the calls above. */
orbfe_status orbfe_cloud_pose_matrix(const float Tcw[16], double out[16]);

/* ---- The fork's 3-D objects (csrc/orbfe_objects.hip) -------------------------------------------------------
 * What viewer() does per keyframe and detected box (src/pointcloudmapping.cc:441-479): ExtractIndices with the indices
 * orbfe_cloud_paint_boxes_device recorded, pcl::StatisticalOutlierRemoval, pcl::VoxelGrid, compute3DCentroid, getMinMax3D; and
 * sem_merge with the `clusters` vector (:246-322).  Bit-exact against tests/objects_oracle.py (unpinned, assumptions O1 .. O12
 * there).  Three decisions are the library's: sqrt(nn_dists[k]) is the DOUBLE square root of the widened float; an object with
 * fewer than mean_k + 1 finite points is reported ORBFE_OBJECT_TOO_FEW, not filtered, and yields no cluster (the reference reads
 * past the end of an array there); an object with no index or no voxel is reported ORBFE_OBJECT_EMPTY and yields no cluster.
 * The calls hang off an orbfe_cloud handle; their scratch is allocated at their first use.  mean_k in [1, 63] (the reference: 50),
 * stddev_mul a number (the reference: 1.0), mode = how the nearest neighbours are found (same result): anything else is
 * ORBFE_ERR_ARG before any launch. */
enum { ORBFE_OBJECT_OK = 0, ORBFE_OBJECT_TOO_FEW = 1, ORBFE_OBJECT_EMPTY = 2 };
enum { ORBFE_KNN_AUTO = 0, ORBFE_KNN_BRUTE = 1, ORBFE_KNN_GRID = 2 };
#define ORBFE_OBJECT_CLASSES 21 /* background + the 20 VOC classes */
typedef struct orbfe_object {
    int32_t status, n_in, n_kept, n_voxels; /* indices in, points the filter kept, voxels of the kept points */
    float centroid[3], min[3], max[3];      /* over the voxels; zeros unless status is ORBFE_OBJECT_OK */
    int32_t reserved_;
    double threshold, mean, stddev;         /* of the filter's mean neighbour distances */
} orbfe_object;
typedef struct orbfe_filter_stat {
    int32_t status, n_in, n_finite, n_kept;
    double threshold, mean, stddev;
} orbfe_filter_stat;
/* how one point set's neighbours were found: used = ORBFE_KNN_BRUTE or ORBFE_KNN_GRID; for the grid its cells per axis, its
 * origin and cells per metre: the cell of x is min(dims[0] - 1, (int)((x - origin[0]) * inv_cell)), in float.  The grid depends
 * on the set's bounds and its number of finite points only. */
typedef struct orbfe_knn_plan {
    int32_t used, dims[3];
    float origin[3], inv_cell;
    int32_t n_finite, cells;
} orbfe_knn_plan;
/* pcl::StatisticalOutlierRemoval over nobj point sets at once: set o is d_points[offsets[o] .. offsets[o + 1]) (offsets: HOST,
 * nobj + 1 entries from 0).  d_distances (one float per record) receives the mean distance to the mean_k nearest neighbours (0 for
 * a record that is not finite and for the sets that are not filtered), d_keep (one byte per record) 1 for a point that stays;
 * stats [nobj] and, unless NULL, plans [nobj] are HOST arrays. */
orbfe_status orbfe_cloud_outlier_filter_device(orbfe_cloud *h, const orbfe_cloud_point *d_points, const int32_t *offsets, int32_t nobj,
                                               int32_t mean_k, double stddev_mul, int32_t mode, float *d_distances, uint8_t *d_keep,
                                               orbfe_filter_stat *stats, orbfe_knn_plan *plans, void *stream);
/* The objects of ONE keyframe: the depth plane, the colour plane orbfe_cloud_paint_boxes_device painted, intrinsics [4] and T [16]
 * as for orbfe_cloud_generate_device, and that call's d_indices (device) and counts [nboxes] (host).  objects [nboxes] (HOST) is
 * filled.  Unless NULL, d_kept receives the flat indices the filter kept (box after box, objects[b].n_kept each) and d_voxels the
 * voxel records (objects[b].n_voxels each, the objects that are not OK have none); *n_kept / *n_voxels = their totals.  More than
 * kept_cap / voxel_cap: ORBFE_ERR_CAP, the totals report the need, nothing else is written.  An index outside the plane yields a
 * point that is not finite. */
orbfe_status orbfe_cloud_objects_device(orbfe_cloud *h, const float *d_depth, size_t depth_stride, const uint8_t *d_bgr, size_t bgr_stride,
                                        const float *intrinsics, const double *T, const int32_t *d_indices, const int32_t *counts,
                                        int32_t nboxes, int32_t mean_k, double stddev_mul, int32_t mode, orbfe_object *objects,
                                        int32_t *d_kept, int32_t kept_cap, orbfe_cloud_point *d_voxels, int32_t voxel_cap, int32_t *n_kept,
                                        int32_t *n_voxels, void *stream);
/* one keyframe from HOST planes (no padding) and HOST boxes / colours as for orbfe_cloud_paint_boxes_device, on the handle's
 * stream: the paint (bgr is painted in place), then the objects */
orbfe_status orbfe_cloud_objects(orbfe_cloud *h, const float *depth, uint8_t *bgr, const float *intrinsics, const double *T,
                                 const float *boxes, const uint8_t *colors, int32_t nboxes, int32_t mean_k, double stddev_mul, int32_t mode,
                                 orbfe_object *objects);
/* bytes of device scratch the calls of this section have allocated on the handle so far (0 until the first of them) */
int64_t orbfe_cloud_objects_scratch_bytes(const orbfe_cloud *h);
/* Host only: the reference's `clusters` vector and sem_merge.  obj_size [ORBFE_OBJECT_CLASSES] = the distance below which two
 * centroids of a class are one object, NULL = the reference's table.  merge: the nearest same-class entry closer than 100 m and
 * than obj_size[class_id] takes the cluster (prob and centroid averaged, min the smaller minimum, max the SMALLER maximum, as
 * the reference has it), else it is appended; *index_out = the entry.  The caller applies the reference's prob > 0.54 gate and
 * merges only objects whose status is ORBFE_OBJECT_OK. */
typedef struct orbfe_cluster {
    int32_t class_id;
    float prob, centroid[3], min[3], max[3];
} orbfe_cluster;
typedef struct orbfe_objects orbfe_objects;
orbfe_status orbfe_objects_create(const float *obj_size, orbfe_objects **out);
void orbfe_objects_destroy(orbfe_objects *db);
orbfe_status orbfe_objects_merge(orbfe_objects *db, int32_t class_id, float prob, const float *centroid, const float *min_pt,
                                 const float *max_pt, int32_t *index_out);
int32_t orbfe_objects_size(const orbfe_objects *db);
orbfe_status orbfe_objects_get(const orbfe_objects *db, int32_t i, orbfe_cluster *out);
void orbfe_objects_clear(orbfe_objects *db);

/* ---- PnPsolver's EPnP RANSAC (csrc/orbfe_pnp.hip) ----------------------------------------------------------
 * The reference's PnPsolver (src/PnPsolver.cc): EPnP on four correspondences inside the RANSAC loop of `iterate`, with Refine's
 * EPnP over the best inliers, the step of Tracking::Relocalization between SearchByBoW and PoseOptimization.  The inputs are the
 * constructor's vectors of the N correspondences: P3Dw [N][3] (map point positions), P2D [N][2] (undistorted keypoints), sigma2
 * [N] (mvLevelSigma2 of the keypoint's octave), float; K = (fx, fy, cx, cy).  The random draws are an input: raw values in
 * [0, 2^31 - 1], FOUR per iteration, index (int)(((double)r / 2147483648.0) * size) over the shrinking list; Refine consumes none.
 * Everything is the reference's arithmetic, fp64 where it uses double and float where it uses float, bit-exact against
 * tests/pnp_oracle.py (an unpinned restatement; its numbered assumptions P1.. are DESIGN 8h's). */
typedef struct orbfe_pnp_params {
    int32_t min_inliers;            /* mRansacMinInliers after SetRansacParameters */
    int32_t max_its;                /* mRansacMaxIts, clamped */
    float epsilon;                  /* mRansacEpsilon, possibly raised */
    float th2;                      /* mvMaxError[i] = sigma2[i] * th2; orbfe_pnp_ransac_params sets the reference's default 5.991 */
} orbfe_pnp_params;
typedef struct orbfe_pnp_state {    /* what a solver carries from one iterate call to the next; all zero = a new solver */
    int32_t iterations;             /* mnIterations */
    int32_t best_inliers;           /* mnBestInliers */
    int32_t reserved[2];
    float best_Tcw[16];             /* mBestTcw */
} orbfe_pnp_state;
typedef struct orbfe_pnp_result {
    int32_t found;                  /* a pose was returned: Refine's (refined = 1) or, at the clamp, the best one (refined = 0) */
    int32_t no_more;                /* bNoMore */
    int32_t n_inliers;              /* nInliers, 0 unless found */
    int32_t iterations_run;         /* iterations this call ran = groups of four draws it consumed */
    int32_t refined;
    int32_t refine_runs;            /* EPnP runs of Refine in this call: one per best mask (a failed Refine is a function of the best
                                       mask alone and is not repeated until the best changes), where the reference runs one per
                                       iteration at or above min_inliers */
    int32_t reserved[2];
    float Tcw[16];                  /* the returned matrix, all zeros unless found */
} orbfe_pnp_result;
typedef struct orbfe_pnp_set {      /* one set of the batched form */
    float K[4];
    orbfe_pnp_params params;
    int32_t n_iterations;           /* iterate's argument */
    int32_t draws_offset;           /* first draw of the set in d_draws */
    int32_t key_offset, n_keys;     /* the set's slice of d_key_mask (n_keys = 0: no scatter) */
} orbfe_pnp_set;
typedef struct orbfe_pnp_iter {     /* tap record of one iteration run */
    int32_t quad[4];                /* the four correspondences drawn */
    int32_t N;                      /* compute_pose's choice among the three beta approximations, 1 .. 3 */
    int32_t n_inliers;              /* mnInliersi */
    int32_t refine_ran;             /* this call ran Refine's EPnP at this iteration */
    int32_t refine_inliers;         /* mnRefinedInliers of the best mask of this iteration, 0 when n_inliers < min_inliers */
    double R[9], t[3];              /* mRi, mti */
} orbfe_pnp_iter;
typedef struct orbfe_pnp orbfe_pnp;   /* device scratch for one host call and for Refine, test taps, own stream */
/* max_points: correspondences of one host call, and of all sets of one batched call together */
orbfe_status orbfe_pnp_create(int32_t device, int32_t max_points, int32_t max_sets, orbfe_pnp **out);
void orbfe_pnp_destroy(orbfe_pnp *h);
void *orbfe_pnp_get_stream(orbfe_pnp *h);
/* Host only: SetRansacParameters as written (the N * epsilon truncation, both clamps, the epsilon raise, pow(epsilon, 3) although
 * the set is 4, the host's libm); out->th2 = 5.991. */
orbfe_status orbfe_pnp_ransac_params(double probability, int32_t min_inliers, int32_t max_its, int32_t min_set, float epsilon, int32_t n,
                                     orbfe_pnp_params *out);
/* iterations one call can run: the reference's loop goes on while mnIterations < mRansacMaxIts OR nCurrentIterations <
 * n_iterations, i.e. max(n_iterations, max_its - state->iterations) unless Refine returns first.  The call reads 4 draws for
 * each of them. */
int32_t orbfe_pnp_iterations(const orbfe_pnp_state *state, const orbfe_pnp_params *params, int32_t n_iterations);
/* One solver's iterate(n_iterations) on HOST arrays, synchronous.  draws: 4 * orbfe_pnp_iterations(..) values.  state and
 * best_mask (mvbBestInliers, uint8 [n]) are the solver's, in / out; mask (may be NULL) is vbInliers per correspondence.  n <
 * min_inliers gives no_more = 1 and no model, and so does n < 4, where the reference is undefined: the library's decision.
 * ORBFE_ERR_ARG: a NULL pointer, n < 0 or > max_points, negative counters, more iterations than 2^20. */
orbfe_status orbfe_pnp_iterate(orbfe_pnp *h, const float *P3Dw, const float *P2D, const float *sigma2, int32_t n, const float *K,
                               const orbfe_pnp_params *params, int32_t n_iterations, const int32_t *draws, orbfe_pnp_state *state,
                               uint8_t *best_mask, orbfe_pnp_result *result, uint8_t *mask);
/* Batched form, DEVICE buffers: the solvers of one Relocalization round in one launch, one workgroup per set.  Set i holds
 * correspondences [d_offsets[i], d_offsets[i + 1]) of the flat arrays (at most max_points in all).  d_keypoint_index (with
 * d_key_mask, both or neither): mvKeyPointIndices; on a return the set's inliers are scattered into its slice of d_key_mask,
 * which lines up with the vpMapPointMatches the following SearchByProjection takes.  Enqueued on `stream` (NULL = HIP's default
 * stream), no synchronisation. */
orbfe_status orbfe_pnp_iterate_device(orbfe_pnp *h, const int32_t *d_offsets, const float *d_P3Dw, const float *d_P2D,
                                      const float *d_sigma2, const orbfe_pnp_set *d_sets, const int32_t *d_draws, int32_t nsets,
                                      orbfe_pnp_state *d_state, uint8_t *d_best_mask, orbfe_pnp_result *d_result, uint8_t *d_mask,
                                      const int32_t *d_keypoint_index, uint8_t *d_key_mask, void *stream);
/* The constructor on DEVICE data: d_keys the frame's undistorted keypoints (mvKeysUn, ORBFE keypoint records of 28 bytes, pt and
 * octave are read), d_level_sigma2 [n_levels] (mvLevelSigma2), d_mappoint_index [n_keys] the map point of each keypoint (-1 =
 * none or bad; an index >= n_mappoints or an octave outside the levels counts as none), d_mappoint_pos [n_mappoints][3]
 * (GetWorldPos).  Writes mvP2D, mvSigma2, mvP3Dw and mvKeyPointIndices compacted in keypoint order, at most `capacity` of them,
 * and *d_count.  One launch on `stream`, no synchronisation. */
orbfe_status orbfe_pnp_prepare_device(orbfe_pnp *h, const void *d_keys, int32_t n_keys, const float *d_level_sigma2, int32_t n_levels,
                                      const int32_t *d_mappoint_index, const float *d_mappoint_pos, int32_t n_mappoints, float *d_P2D,
                                      float *d_sigma2, float *d_P3Dw, int32_t *d_keypoint_index, int32_t *d_count, int32_t capacity,
                                      void *stream);
/* Test taps, as orbfe_sim3_tap: allocated by the first orbfe_pnp_set_tap_iteration, then recorded for the first
 * ORBFE_PNP_TAP_SETS sets of every call:
 *   0 ORBFE_PNP_TAP_ITERATIONS  one orbfe_pnp_iter per iteration run (the first ORBFE_PNP_TAP_ITERS of them); *count = records
 *   1 ORBFE_PNP_TAP_ERRORS      error2 of CheckInliers, float [n], of the iteration (counted within the call) chosen with
 *                               orbfe_pnp_set_tap_iteration BEFORE the call (default 0); ORBFE_ERR_STATE if it was not run */
#define ORBFE_PNP_TAP_SETS 32
#define ORBFE_PNP_TAP_ITERS 512
enum { ORBFE_PNP_TAP_ITERATIONS = 0, ORBFE_PNP_TAP_ERRORS = 1 };
orbfe_status orbfe_pnp_set_tap_iteration(orbfe_pnp *h, int32_t iteration);
orbfe_status orbfe_pnp_tap(orbfe_pnp *h, int32_t set, int32_t stage, void *dst, size_t cap, int32_t *count);
/* Known-answer runs of the device primitives on the caller's current device, doubles in and out, n items:
 *   0..4  SVD of a 3x3 / 12x12 / 6x3 / 6x4 / 6x5 matrix (row-major): out = w [k], the left vectors as rows [k][m], the right
 *         vectors as rows [k][k] -- OpenCV 3.2's JacobiSVDImpl_<double>
 *   5..7  cvSolve(A, b, CV_SVD) on 6x3 / 6x4 / 6x5: in = A, b [6]; out = x [k]
 *   8     cvInvert(A, CV_SVD) on 3x3
 *   9     qr_solve on 6x4: in = A, b [6]; out = x [4], left at zeros when a column is found all zero
 *   10    compute_pose on n correspondences (ONE item): in = fu, fv, uc, vc, then n x (X, Y, Z, u, v); out = R [9], t [3], the
 *         error returned, N, the three rep_errors */
enum {
    ORBFE_PNP_KAT_SVD3 = 0, ORBFE_PNP_KAT_SVD12 = 1, ORBFE_PNP_KAT_SVD6X3 = 2, ORBFE_PNP_KAT_SVD6X4 = 3, ORBFE_PNP_KAT_SVD6X5 = 4,
    ORBFE_PNP_KAT_SOLVE6X3 = 5, ORBFE_PNP_KAT_SOLVE6X4 = 6, ORBFE_PNP_KAT_SOLVE6X5 = 7, ORBFE_PNP_KAT_INVERT3 = 8,
    ORBFE_PNP_KAT_QR_SOLVE = 9, ORBFE_PNP_KAT_COMPUTE_POSE = 10
};
orbfe_status orbfe_pnp_kat(int32_t what, int32_t n, const double *in, double *out);

/* ---- the monocular Initializer (csrc/orbfe_initializer.hip) ---------------------------------------------------
 * ORB_SLAM2::Initializer::Initialize of src/Initializer.cc: the H / F RANSAC over `iterations` sets of eight matches, the model
 * choice by RH = SH / (SH + SF) > 0.40, ReconstructH (8 hypotheses) or ReconstructF (4), CheckRT with Triangulate, and the
 * final ladder.  The random draws are an INPUT: iterations x 8 raw rand() values, turned into mvSets as the reference does
 * (RandomInt on the shrinking list, swap with back).  Bit-exact against tests/initializer_oracle.py (an unpinned restatement;
 * its numbered assumptions I1.. are DESIGN 8j's).  K is the 3 x 3 calibration matrix, row-major. */
typedef struct orbfe_initializer_result {
    int32_t ok;              /* what Initialize returns */
    int32_t status;          /* ORBFE_INIT_*: why nothing ran, 0 if the chain ran */
    int32_t model;           /* 0 none, 1 H (RH > 0.40), 2 F */
    int32_t n_matches;       /* N = matches12 entries >= 0 */
    float SH, SF;            /* the best scores; 0 when no iteration had a positive one */
    int32_t iterH, iterF;    /* the iterations that won (strict >, so the first of equal scores), -1 if none */
    float H21[9], F21[9];    /* their models, zeros if none */
    float R21[9], t21[3];    /* zeros unless ok */
    int32_t n_hyp;           /* hypotheses CheckRT ran on: 8, 4, or 0 at ReconstructH's d1/d2, d2/d3 early-out */
    int32_t nGood[8];
    int32_t n_cos[8];        /* size of vCosParallax per hypothesis */
    float sel_cos[8];        /* vCosParallax[min(50, size - 1)] after the sort; 0 where nGood = 0 */
    int32_t best;            /* H: bestSolutionIdx; F: the first hypothesis with maxGood; -1 if none */
    int32_t second;          /* H: secondBestGood; F: nsimilar */
    int32_t n_inliers;       /* N of ReconstructH / ReconstructF: the winner's inliers */
    int32_t parallax_ok;     /* the best hypothesis's parallax test (> 1 for F, >= 1 for H), as a cut on sel_cos[best] */
    float parallax_cos;      /* sel_cos[best] */
    float parallax;          /* acosf(parallax_cos) * 180 / pi with the device's acosf: reported, never decided on */
    int32_t reserved[3];
} orbfe_initializer_result;   /* 72 words */
typedef struct orbfe_initializer_pair {   /* one frame pair of the batched form */
    float K[9];
    float sigma;
    int32_t iterations;      /* 1 .. ORBFE_INIT_MAX_ITERATIONS */
    int32_t draws_offset;    /* into d_draws, in values; iterations * 8 are read */
    int32_t reserved[4];
} orbfe_initializer_pair;     /* 16 words */
typedef struct orbfe_initializer_iter {   /* tap record of one iteration */
    int32_t set[8];          /* mvSets[it]: indices into the compacted match list */
    float Hn[9], Fn[9];      /* ComputeH21 / ComputeF21 on the normalised points */
    float H21i[9], F21i[9];
    float scoreH, scoreF;
    int32_t reserved[2];
} orbfe_initializer_iter;     /* 48 words */
enum { ORBFE_INIT_OK = 0, ORBFE_INIT_FEW_MATCHES = 1, ORBFE_INIT_BAD_INDEX = 2, ORBFE_INIT_NO_MODEL = 3, ORBFE_INIT_BAD_SIZES = 4 };
#define ORBFE_INIT_MAX_ITERATIONS 512
#define ORBFE_INIT_TAP_SETS 32
#define ORBFE_INIT_TAP_ITERS 512
#define ORBFE_INIT_ERR_FLOATS 9
typedef struct orbfe_initializer orbfe_initializer;
/* Device scratch for calls of at most max_matches keys of the first frames (all pairs of a batch together; the compacted match
 * lists live there) and max_pairs pairs, with a stream of its own. */
orbfe_status orbfe_initializer_create(int32_t device, int32_t max_matches, int32_t max_pairs, orbfe_initializer **out);
void orbfe_initializer_destroy(orbfe_initializer *h);
void *orbfe_initializer_get_stream(orbfe_initializer *h);
/* One Initialize on HOST arrays, synchronous: one launch sequence and one synchronisation on the handle's stream.  keys*_xy
 * float [n][2] (mvKeysUn's pt), matches12 int32 [n1] (index into keys2, < 0 = none), K float [9], draws int32 [iterations * 8].
 * Out: *result, P3D float [n1][3], triangulated uint8 [n1] (zeros unless ok).  Fewer than 8 matches, a match index >= n2,
 * iterations outside 1 .. ORBFE_INIT_MAX_ITERATIONS, n1 > max_matches: ORBFE_ERR_ARG (undefined in the reference). */
orbfe_status orbfe_initializer_initialize(orbfe_initializer *h, const float *keys1_xy, int32_t n1, const float *keys2_xy, int32_t n2,
                                          const int32_t *matches12, const float *K, float sigma, int32_t iterations,
                                          const int32_t *draws, orbfe_initializer_result *result, float *P3D, uint8_t *triangulated);
/* Many pairs in one call on the caller's stream, everything in device memory, no synchronisation: d_offsets1 / d_offsets2 int32
 * [npairs + 1] are the CSR offsets of the pairs' keys in d_keys1_xy / d_keys2_xy; d_matches12, d_P3D, d_triangulated follow
 * d_offsets1 (the matches can be a row of the device matcher's output block as it stands: -1 = none).  A pair the host form
 * would have refused gets result.status != 0 and ok = 0; nothing else of it is written.  The host reads only the pointers.
 * A pair without keys in either frame (n1 = 0 or n2 = 0, its matches all < 0) is ORBFE_INIT_FEW_MATCHES like any pair of fewer
 * than 8 matches: its (possibly empty) slices of d_P3D / d_triangulated keep what they held.  A pair fits when offsets1[p + 1] <=
 * max_matches: a batch may end exactly at max_matches; a pair that ends past it is ORBFE_INIT_BAD_SIZES, the pairs before it run.
 * Pairs may differ in `iterations` (1 .. ORBFE_INIT_MAX_ITERATIONS side by side), and a handle may run batches of any order and
 * size one after the other: a pair reads only what the same call wrote into the handle's scratch. */
orbfe_status orbfe_initializer_initialize_device(orbfe_initializer *h, const int32_t *d_offsets1, const int32_t *d_offsets2,
                                                 const float *d_keys1_xy, const float *d_keys2_xy, const int32_t *d_matches12,
                                                 const orbfe_initializer_pair *d_pairs, const int32_t *d_draws, int32_t npairs,
                                                 orbfe_initializer_result *d_result, float *d_P3D, uint8_t *d_triangulated,
                                                 void *stream);
/* Test taps, as orbfe_pnp_tap: allocated by the first orbfe_initializer_set_tap_iteration, then recorded for the first
 * ORBFE_INIT_TAP_SETS pairs of every call:
 *   0 ORBFE_INIT_TAP_ITERATIONS  one orbfe_initializer_iter per iteration; *count = records
 *   1 ORBFE_INIT_TAP_MATCHES     float [N][9] per compacted match: chiSquare1, chiSquare2 of CheckHomography and of
 *                                CheckFundamental for the models of iteration `iteration`, then p3dC1 [3], cosParallax and the
 *                                stage at which CheckRT dropped the match (ORBFE_INIT_RT_*, as a float) for hypothesis
 *                                `hypothesis`, both chosen BEFORE the call; ORBFE_ERR_STATE if that iteration did not run
 * A pair at or past ORBFE_INIT_TAP_SETS (or past the handle's max_pairs, or of no call yet) has no tap: ORBFE_ERR_STATE; its
 * result, points and flags are those of any other pair.  ORBFE_INIT_TAP_ITERS = ORBFE_INIT_MAX_ITERATIONS: every iteration of
 * a tapped pair has its record.  A NaN in a tap is a NaN of the reference's arithmetic at that place; its payload is not. */
enum { ORBFE_INIT_TAP_ITERATIONS = 0, ORBFE_INIT_TAP_MATCHES = 1 };
enum {
    ORBFE_INIT_RT_OUTLIER = 0, ORBFE_INIT_RT_NONFINITE = 1, ORBFE_INIT_RT_DEPTH1 = 2, ORBFE_INIT_RT_DEPTH2 = 3, ORBFE_INIT_RT_ERROR1 = 4,
    ORBFE_INIT_RT_ERROR2 = 5, ORBFE_INIT_RT_FAR = 6, ORBFE_INIT_RT_GOOD = 7
};
orbfe_status orbfe_initializer_set_tap_iteration(orbfe_initializer *h, int32_t iteration, int32_t hypothesis);
orbfe_status orbfe_initializer_tap(orbfe_initializer *h, int32_t pair, int32_t stage, void *dst, size_t cap, int32_t *count);
/* Known-answer runs of the device primitives on the caller's current device, floats in and out, n items:
 *   0..3  cv::SVD::compute(FULL_UV) of a 16x9 / 8x9 / 3x3 / 4x4 CV_32F matrix (row-major): out = w [min], u [rows][rows],
 *         vt [cols][cols] -- OpenCV 3.2's JacobiSVDImpl_<float>; for 8x9 vt row 8 is the RNG refill row
 *   4     Mat::inv() of a 3x3
 *   5, 6  ComputeH21 / ComputeF21: in = vP1 [8][2], vP2 [8][2]; out = [9]
 *   7     Triangulate: in = kp1 xy, kp2 xy, P1 [12], P2 [12]; out = x3D [3]
 *   8     the parallax cut: in = one cosine; out = 1 or 0 */
enum {
    ORBFE_INIT_KAT_SVD16X9 = 0, ORBFE_INIT_KAT_SVD8X9 = 1, ORBFE_INIT_KAT_SVD3 = 2, ORBFE_INIT_KAT_SVD4 = 3, ORBFE_INIT_KAT_INV3 = 4,
    ORBFE_INIT_KAT_H21 = 5, ORBFE_INIT_KAT_F21 = 6, ORBFE_INIT_KAT_TRIANGULATE = 7, ORBFE_INIT_KAT_PARALLAX = 8
};
orbfe_status orbfe_initializer_kat(int32_t what, int32_t n, const float *in, float *out);

/* ---- the fork's multi-view geometry dynamic-point mask (csrc/orbfe_geometry.hip) -------------------------
 * DynaSLAM::Geometry (perfect/src/Geometry.cc): the key-frame ring of DataBase::InsertFrame2DB (:532-550, 20 slots, mNumElem stops
 * at 19 and GetRefFrames reads slots 0 .. mNumElem-1 whatever mIni / mFin say), GetRefFrames (:83-127, host only, rotm2euler's
 * at<double> read of the CV_32F pose kept as it behaves), ExtractDynPoints (:136-471), RegionGrowing (:604-700),
 * DepthRegionGrowing (:475-518, any w x h with w, h >= 45 instead of the hard-coded 640 x 480) and GeometricModelCorrection
 * (:50-69).  Every operation in the reference's type and order, OpenCV 3.2's MatExpr / gemm / solve / meanStdDev arithmetic
 * restated; acos is a fixed fp64 operation sequence (fdlibm's), not a C library's.  Bit-exact against tests/geometry_oracle.py
 * (an unpinned restatement of OpenCV 3.2).  Depth planes are float, finite and >= 0: a non-finite depth is outside the contract.
 * A key-frame keypoint outside its depth plane (x > -1 && x < w && y > -1 && y < h decides, in float) is dropped; the reference
 * reads the plane unchecked.  Poses are 16 floats, row-major mTcw. */
typedef struct orbfe_geometry orbfe_geometry;   /* one DynaSLAM::Geometry: own stream, the device-resident key-frame ring, scratch */
#define ORBFE_GEOMETRY_DB_SIZE 20      /* MAX_DB_SIZE */
#define ORBFE_GEOMETRY_REF_FRAMES 5    /* MAX_REF_FRAMES and ELEM_INITIAL_MAP */
orbfe_status orbfe_geometry_create(int32_t device, int32_t max_w, int32_t max_h, int32_t max_keypoints, int32_t max_seeds,
                                   orbfe_geometry **out);
void orbfe_geometry_destroy(orbfe_geometry *g);
orbfe_status orbfe_geometry_reset(orbfe_geometry *g);   /* an empty ring */
void *orbfe_geometry_get_stream(orbfe_geometry *g);
/* GeometricModelUpdateDB for a frame the caller declares a key frame: depth plane (w x h floats, rows depth_stride BYTES apart),
 * mvKeys, mvKeysUn (n of each, n <= max_keypoints) and mTcw go into the ring slot InsertFrame2DB writes.  on_device != 0: depth,
 * kps and kps_un are DEVICE pointers (Tcw is always host).  Synchronous; waits for the last correct call first. */
orbfe_status orbfe_geometry_insert_keyframe(orbfe_geometry *g, const float *depth, int32_t w, int32_t h, size_t depth_stride,
                                            const orbfe_keypoint *kps, const orbfe_keypoint *kps_un, int32_t n, const float *Tcw,
                                            int32_t on_device);
/* the ring's mNumElem, mIni, mFin and, per slot, how many inserts came before the one it holds (-1: never written; slot [20]) */
orbfe_status orbfe_geometry_db_state(orbfe_geometry *g, int32_t *num_elem, int32_t *ini, int32_t *fin, int32_t *slot_insert);
/* GetRefFrames, host only, no device needed: db_Tcw [n][16], n <= 20; idx receives min(5, n) slot numbers, most distant first
 * (0.7 * |dt| / max + 0.3 * |deuler| / max, descending).  Equal scores are outside the contract (cv::sortIdx is not stable). */
orbfe_status orbfe_geometry_select_ref_frames(const float *cur_Tcw, const float *db_Tcw, int32_t n, int32_t *idx, int32_t *nref);
/* GeometricModelCorrection on one HOST depth plane: HOST mask (w x h, rows mask_stride bytes apart, 1 = static, 0 = dynamic).
 * Fewer than 5 key frames, or Tcw == NULL (the empty pose): the mask is all ones and *computed = 0 (the reference leaves its
 * mask alone); else *computed = 1.  Synchronous. */
orbfe_status orbfe_geometry_correct(orbfe_geometry *g, const float *depth, int32_t w, int32_t h, size_t depth_stride, const float *Tcw,
                                    float fx, float fy, float cx, float cy, uint8_t *mask, int32_t mask_stride, int32_t *computed);
/* nframes current frames (DEVICE depth planes, frame f at d_depth + f * depth_frame_stride bytes; HOST poses [nframes][16], read
 * before the call returns) against the ring as it stands.  d_mask [nframes] and d_mask_ones (the count of ones, may be NULL) in
 * the layout orbfe_mask_keypoints_device reads; computed: HOST [nframes], written before the call returns (may be NULL).
 * Enqueued on `stream`, no synchronisation and no host read between the stages: the dynamic-point count stays on the device,
 * seeds beyond max_seeds are grown in ordered passes that carry the union. */
orbfe_status orbfe_geometry_correct_batch_device(orbfe_geometry *g, const float *d_depth, int32_t nframes, int32_t w, int32_t h,
                                                 size_t depth_stride, size_t depth_frame_stride, const float *Tcw, float fx, float fy,
                                                 float cx, float cy, uint8_t *d_mask, int32_t mask_stride, size_t mask_frame_stride,
                                                 int32_t *d_mask_ones, int32_t *computed, void *stream);
/* DepthRegionGrowing alone on one HOST depth plane and n seeds (x, y) int32 pairs in order (n <= 5 * max_keypoints, every seed
 * inside the plane): HOST mask out.  The taps below (frame 0) then show the accepted seeds, the union and the regions. */
orbfe_status orbfe_geometry_depth_region_growing(orbfe_geometry *g, const float *depth, int32_t w, int32_t h, size_t depth_stride,
                                                 const int32_t *seeds_xy, int32_t n, uint8_t *mask, int32_t mask_stride);
/* Test taps of the last correct / region-growing call (synchronises its stream).  `frame` counts within the call's last chunk
 * of frames (orbfe_geometry_chunk frames at most); ORBFE_ERR_STATE for a frame that chunk did not hold or did not compute.
 *   0 ORBFE_GEOMETRY_TAP_COUNTS  int32 [8]: reference keypoints read, then the survivors of 0 < d < 6, of the parallax gate, of
 *                                depth < 7, of IsInFrame and depth > 0, of the 41x41 search, of the 0.6 gate, of the variance gate
 *   1 ORBFE_GEOMETRY_TAP_DYN     int32 [*count][3]: the dynamic points (x, y, label) in the reference's order
 *   2 ORBFE_GEOMETRY_TAP_SEEDS   uint8 [*count]: 1 where DepthRegionGrowing grew the seed
 *   3 ORBFE_GEOMETRY_TAP_UNION   uint8 [h][w]: the union before the dilation; *count = w * h
 *   4 ORBFE_GEOMETRY_TAP_REGION  uint8 [h][w]: RegionGrowing's J of seed `index` of the LAST pass that had seeds (index <
 *                                max_seeds; all zero for a seed DepthRegionGrowing skipped); *count = w * h */
enum { ORBFE_GEOMETRY_TAP_COUNTS = 0, ORBFE_GEOMETRY_TAP_DYN = 1, ORBFE_GEOMETRY_TAP_SEEDS = 2, ORBFE_GEOMETRY_TAP_UNION = 3,
       ORBFE_GEOMETRY_TAP_REGION = 4 };
orbfe_status orbfe_geometry_tap(orbfe_geometry *g, int32_t frame, int32_t stage, int32_t index, void *dst, size_t cap, int32_t *count);
int32_t orbfe_geometry_chunk(orbfe_geometry *g);   /* frames per internal pass of the batch form */
/* host constants, no device needed: the half-widths of getStructuringElement(MORPH_ELLIPSE, (2r+1, 2r+1)), rows 0 .. 2r */
orbfe_status orbfe_geometry_ellipse(int32_t r, int32_t *half_width);
/* Known-answer runs on the caller's current device, n doubles in and out: 0 = the canonical acos */
enum { ORBFE_GEOMETRY_KAT_ACOS = 0 };
orbfe_status orbfe_geometry_kat(int32_t what, int32_t n, const double *in, double *out);

#ifdef __cplusplus
}
#endif
#endif /* ORBFE_H */
