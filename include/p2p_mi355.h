/*
 * p2p_mi355.h -- C ABI of libp2p_mi355.so: the MI355X (gfx950) drop-in for the Pix2Pose
 * inference hot path.  Plain pointers and sizes only; no torch / numpy / C++ types.
 *
 * Every entry point names the reference interface (kirumang/Pix2Pose, file:line) it
 * replaces.  All functions return P2P_OK (0) or a negative p2p_status; they never throw or
 * abort.  p2p_last_error() gives a human-readable reason for the calling thread.
 *
 * Threading: a p2p_ctx owns one HIP stream and its workspaces and is NOT thread-safe;
 * different contexts (one per GPU / rank) are independent.
 */
#ifndef P2P_MI355_H
#define P2P_MI355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P2P_ABI_VERSION 12

/* The library is built with -fvisibility=hidden: the entry points declared here (P2P_API) are its ONLY dynamic symbols
 * (tests/test_host_cpu.py holds `nm -D` to exactly this list). */
#if defined(__GNUC__)
#define P2P_API __attribute__((visibility("default")))
#else
#define P2P_API
#endif

typedef enum {
    P2P_OK = 0,
    P2P_ERR_INVALID_ARG = -1,   /* null pointer, bad size, unknown enum */
    P2P_ERR_HIP = -2,           /* a HIP runtime call failed (no GPU, OOM, launch failure) */
    P2P_ERR_WEIGHTS = -3,       /* missing / mis-sized weight tensor */
    P2P_ERR_CAPACITY = -4,      /* request exceeds a capacity fixed at ctx creation */
    P2P_ERR_RANGE = -5          /* a P2P_PREC_F16X3 generator pass stored an activation beyond the split-f16 operand range (see p2p_precision) */
} p2p_status;

/* reference: recognition.py:21-26 selects the generator graph from the `backbone` string */
typedef enum { P2P_BACKBONE_PAPER = 0, P2P_BACKBONE_RESNET50 = 1 } p2p_backbone;

/* where a caller buffer lives */
typedef enum { P2P_MEM_HOST = 0, P2P_MEM_DEVICE = 1 } p2p_mem;

typedef struct p2p_ctx p2p_ctx;     /* per-GPU pipeline context: stream + workspaces      */
typedef struct p2p_model p2p_model; /* one object's generator network, weights in HBM     */

/* One named weight tensor in Keras-native layout (see pix2pose_amd/weights.py):
 * Conv2D (kh,kw,Cin,Cout), Conv2DTranspose (kh,kw,Cout,Cin), Dense (in,out), BN vectors. */
typedef struct {
    const char* name;
    const float* data; /* host pointer */
    int64_t numel;
} p2p_tensor;

P2P_API int p2p_abi_version(void);
/* Binding self-checks: sizeof() of the public structs as this build of the library sees them
 * (which: 0 p2p_tensor, 1 p2p_image, 2 p2p_object, 3 p2p_detection, 4 p2p_pose, 5 p2p_est_pose_opts,
 * 6 p2p_kernel_stats, 7 p2p_refine_job, 8 p2p_depth_score, 9 p2p_icp_input, 10 p2p_icp_params, 11 p2p_icp_result,
 * 12 p2p_refine_result; -1 otherwise), and the hash of the sources the library was built from
 * (pix2pose_amd/build.py) -- a foreign-language binding compares both with its own declarations / tree
 * before the first call, so that a stale .so is an error and not a silent struct mismatch. */
P2P_API int p2p_abi_sizeof(int which);
P2P_API const char* p2p_build_id(void);
/* Test hook, no GPU needed: the one-sided Gaussian weights (centre first) the anti-aliased resize uses for crop side
 * `side` against the 128-px network resolution; w must hold 256 doubles.  Returns the radius (0: no filtering), -1 on a bad
 * side.  tests/ hold it against scipy.ndimage's own kernel bit for bit. */
P2P_API int p2p_aa_weights(int side, double* w);
/* Test hook (GPU): the back-resizes of recognition.py:134,144,146 on caller-supplied 128 x 128 maps through the code the pipeline runs --
 * prob [128*128] (cval 1), pred [128*128*3] (img_pred, cval 0.5), non_gray [128*128] (0 / 1, cval 0), host float32 -- at out_h x out_w;
 * generation = p2p_est_pose_opts.resize_anti_aliasing.  Outputs (host): q [out_h*out_w*3] = (resize(pred) * 255) truncated to uint8,
 * below [out_h*out_w] = resize(prob) < th_inlier, ng_out = resize(non_gray) > 0.9.  tests/test_external_vectors.py holds it against the
 * vectors of the real scikit-image 0.18.3. */
P2P_API int p2p_debug_back_resize(p2p_ctx* ctx, const float* prob, const float* pred, const float* non_gray, int out_h, int out_w,
                                  double th_inlier, int generation, unsigned char* q, unsigned char* below, unsigned char* ng_out);
P2P_API const char* p2p_last_error(void);
P2P_API int p2p_device_count(int* count);

/* Create a context on `device`.  `max_batch` = largest number of 128x128 network inputs
 * processed per pass (activation workspace is sized for it; larger requests are chunked).
 * The est_pose workspaces (correspondences, canvases, landing buffers) are grow-only and sized by the batches
 * that arrive: nothing about frame or crop sizes is fixed here. */
P2P_API int p2p_ctx_create(int device, int max_batch, p2p_ctx** out);
P2P_API void p2p_ctx_destroy(p2p_ctx* ctx);
P2P_API int p2p_ctx_synchronize(p2p_ctx* ctx);
/* HIP stream handle (hipStream_t) the context launches on, for callers that time kernels
 * with HIP events or chain their own work. */
P2P_API void* p2p_ctx_stream(p2p_ctx* ctx);

/* Replaces `ae.aemodel_unet_*(p=1.0)` + `generator_train.load_weights(weight_fn)`
 * (reference recognition.py:21-26; graphs ae_model.py:70-150,175-240): uploads the
 * tensors, folds BatchNorm into per-channel scale/shift and re-packs kernels for the
 * MFMA implicit-GEMM kernels.  All tensors of pix2pose_amd.weights.tensor_specs(backbone)
 * must be present. */
P2P_API int p2p_model_create(p2p_ctx* ctx, const p2p_tensor* tensors, int n_tensors, int backbone,
                     p2p_model** out);

/* Arithmetic of the generator's dense contractions (the reference computes them in fp32 through
 * TensorFlow).  P2P_PREC_F32: fp32 matrix instructions, bitwise an fmaf chain.  P2P_PREC_F16X3: fp32
 * emulated on the f16 matrix pipe -- every operand is split into two f16 halves (22 significant
 * bits), three MFMAs per product block, fp32 accumulation; ~2.7x faster on the large layers, output
 * differs from the fp32 mode by ~1e-6 and is measured as close to a double-accumulating reference as
 * the fp32 mode is (max 2.5e-5 vs 3.3e-5 on the tanh outputs).  Weights are pre-scaled per output channel.
 * OPERAND RANGE of the split: |activation| < 65504 (f16 max).  Batch-normalised layers sit orders of magnitude below; the two
 * linear Dense layers (ae_model.py:199-200) have no BatchNorm behind them.  The range is GUARDED: every layer epilogue tracks the
 * largest magnitude it stores and raises a device-side flag beyond 6e4 -- a NaN counts as beyond (the running maximum and the ReLU of the
 * epilogues propagate NaN); the caller-supplied input x of p2p_predict / p2p_forward_async is NOT checked (|x| < 65504 is the caller's to
 * keep: the pipeline's own inputs are (u8 - 128) / 128) -- the flag travels with the results and
 *   p2p_predict / p2p_est_pose_batch / p2p_est_pose_collect return P2P_ERR_RANGE (outputs / poses of that call are not to be used);
 *   p2p_forward_async cannot report -- ask p2p_ctx_range_event() after synchronising.
 * P2P_PREC_AUTO: split-f16 with a strict-fp32 twin of the same weights kept beside it (+ the model's size in HBM).  On a range event the
 * object switches to the twin for good: p2p_predict and p2p_est_pose_batch repeat the work in fp32 themselves and return P2P_OK;
 * p2p_est_pose_collect returns P2P_ERR_RANGE once and the re-submitted batch runs in fp32.  The flag is per batch, not per object: in a
 * mixed batch every P2P_PREC_AUTO object switches, objects without a twin keep their arithmetic (if one of THOSE overflowed, the repeated
 * batch reports P2P_ERR_RANGE again).  p2p_model_precision() tells which
 * arithmetic an object currently uses.  p2p_model_create uses P2P_PREC_DEFAULT. */
typedef enum { P2P_PREC_F32 = 0, P2P_PREC_F16X3 = 1, P2P_PREC_AUTO = 2 } p2p_precision;
#define P2P_PREC_DEFAULT P2P_PREC_F16X3
P2P_API int p2p_model_create_ex(p2p_ctx* ctx, const p2p_tensor* tensors, int n_tensors, int backbone,
                        int precision, p2p_model** out);
P2P_API void p2p_model_destroy(p2p_model* model);
/* P2P_PREC_F32 or P2P_PREC_F16X3: the arithmetic the object's next pass will use (a P2P_PREC_AUTO object reports F16X3 until a
 * range event switched it to its fp32 twin); negative on a null handle. */
P2P_API int p2p_model_precision(const p2p_model* model);
/* Operand-range events of direct forward calls (p2p_forward_async) since the last query: synchronises the context stream, stores the
 * largest offending magnitude in *max_abs (0 = none) and clears the flag.  No reference counterpart (TensorFlow computes in fp32). */
P2P_API int p2p_ctx_range_event(p2p_ctx* ctx, float* max_abs);

/* Form of the 5x5 layers of the generator in P2P_PREC_F16X3 passes of this context: the stride-1 decoder convolutions deconv1 / deconv2 /
 * deconv3 (reference ae_model.py:207-211,217-220,227-230; 67 % of the generator's multiplications), the transposed convolutions up1 / up2 /
 * up3 (ae_model.py:201-204,212-215,222-225) and the stride-2 convolution conv4 (ae_model.py:190-195).  The Winograd forms along the row
 * axis -- F(4,5) for the stride-1 layers (2.5x fewer matrix-core products), F(4,3) on the sub-pixel phases / parity planes of the stride-2
 * layers (1.67x fewer) -- form different products than the direct convolutions, so the forms do not give the same bits: all are held to the
 * same bar against the oracle (network output within 1e-4; measured 4e-5 with every layer in Winograd form, 2.6e-5 direct;
 * tests/test_wino_gpu.py), 6e-5 apart at most.
 *   P2P_WINOGRAD_AUTO (default)  the fastest form at every pass size: F(4,5) for the stride-1 layers at every size, F(4,3) for up2 / up3 from 5
 *                                and for conv4 / up1 from 9 inputs; launches that would occupy a fraction of the chip split K over more
 *                                workgroups and add the partial sums in a separate step, in a fixed order (a pass over a few inputs: conv4
 *                                on the direct kernel, the stride-1 layers over ranges of channel slices, deconv1 up to 64 inputs; conv4 in
 *                                F(4,3) form over its four parity planes while under one workgroup per CU).  A sample's bits then depend on
 *                                the SIZE of the pass it travels in (never on its content, its order or the run)
 *   P2P_WINOGRAD_OFF             direct forms always   } either way a sample's output bits do not depend on the pass it travels in
 *   P2P_WINOGRAD_ALWAYS          Winograd forms always }  (conv4 split over its parity planes at every size)
 * Strict-fp32 objects (P2P_PREC_F32, the twin of P2P_PREC_AUTO) always use the direct forms.  No reference counterpart. */
typedef enum { P2P_WINOGRAD_OFF = 0, P2P_WINOGRAD_AUTO = 1, P2P_WINOGRAD_ALWAYS = 2 } p2p_winograd_mode;
P2P_API int p2p_ctx_set_winograd(p2p_ctx* ctx, int mode);

/* Replaces `self.generator_train.predict(x)` (reference recognition.py:84,129):
 * x [n,128,128,3] float32 NHWC -> xyz [n,128,128,3] (tanh) and prob [n,128,128,1] (sigmoid).
 * `mem` says whether x/xyz/prob are host or device pointers.  Blocking. */
P2P_API int p2p_predict(p2p_ctx* ctx, const p2p_model* model, const float* x, int n, float* xyz,
                float* prob, int mem);

/* Same forward pass, device buffers only, asynchronous on the context stream, output
 * interleaved [n,128,128,4] = (x,y,z,prob).  Used by the pipeline and by bench.py. */
P2P_API int p2p_forward_async(p2p_ctx* ctx, const p2p_model* model, const float* x_dev, int n,
                      float* xyzp_dev);


/* ------------------------------------------------------------------------------------------
 * Pose estimation: replaces `pix2pose.est_pose(rgb, bbox)` (reference recognition.py:70-193,
 * crop geometry get_boxes :28-69, pnp_ransac :195-224) for a whole batch of detections.
 * ---------------------------------------------------------------------------------------- */
#define P2P_MAX_OUTLIER_TH 8
/* Largest RANSAC iteration count (the reference hard-codes iterationsCount=100, recognition.py:217): the
 * hypothesis storage of the solver is sized for it; larger requests fail with P2P_ERR_INVALID_ARG. */
#define P2P_MAX_RANSAC_ITERATIONS 128

typedef enum { P2P_IMG_U8 = 0, P2P_IMG_F32 = 1 } p2p_img_dtype;

/* One H x W x 3 interleaved RGB frame (`rgb` of est_pose; uint8, or float32 as the ICP script
 * passes, reference tools/5_evaluation_bop_icp3d.py:369-370). */
typedef struct {
    const void* data;
    int height, width;
    int dtype; /* p2p_img_dtype */
    int mem;   /* p2p_mem */
} p2p_image;

/* Per-object state of a reference `pix2pose` instance (recognition.py:10-26): the generator
 * network plus obj_param = [x_scale,y_scale,z_scale,x_ct,y_ct,z_ct] (tools/bop_io.py:33-42),
 * th_outlier (1..8 values, evaluated in order), th_inlier, box_size. */
typedef struct {
    const p2p_model* model;
    double obj_scale[3];
    double obj_ct[3];
    int n_outlier_th;
    double outlier_th[P2P_MAX_OUTLIER_TH];
    double inlier_th;
    double box_size;
} p2p_object;

/* One 2D detection: which frame, which object, bbox = [v_min,u_min,v_max,u_max] (ints, as the
 * detectors hand them over, tools/5_evaluation_bop_basic.py:289-304) and the camera matrix the
 * caller would have assigned to `.camK` before the call (:302). */
typedef struct {
    int image;
    int object;
    int bbox[4];
    double camK[9];
} p2p_detection;

/* est_pose status: the reference signals failure in-band with -1 sentinels (recognition.py:79,
 * 127,191); the shim maps any status != 0 back to those sentinels. */
typedef enum {
    P2P_POSE_RANGE = -2,           /* gathered batches only: a detection of a rank whose batch returned P2P_ERR_RANGE -- it exists, its pose is not to be used */
    P2P_POSE_ABSENT = -1,          /* padding record of a gathered batch (p2p_est_pose_collect_gathered): no detection here */
    P2P_POSE_OK = 0,
    P2P_POSE_CROP_TOO_SMALL = 1,   /* recognition.py:78-79  */
    P2P_POSE_NO_CANDIDATE = 2,     /* recognition.py:125-127 */
    P2P_POSE_PNP_FAILED = 3        /* recognition.py:189-191 */
} p2p_pose_status;

typedef struct {
    double R[9];          /* rot_pred, row-major                           (recognition.py:223) */
    double t[3];          /* tra_pred, mm                                                       */
    double frac_inlier;   /* max_inlier / n_init_mask                      (recognition.py:193) */
    int n_inliers;        /* len(inliers) of the selected candidate                             */
    int n_init_mask;      /* stage-1 non-gray pixel count                  (recognition.py:90)  */
    int status;           /* p2p_pose_status                                                    */
    int best_slot;        /* index into outlier_th of the selected candidate, -1 if none        */
    int bbox_t[4];        /* [v1,v2,u1,u2] as returned by the reference (box of the LAST candidate) */
    int n_candidates;     /* stage-2 candidates that were built                                 */
    int ransac_iters;     /* RANSAC iterations run for the selected candidate                   */
    int64_t mask_stats[3];/* score_type 2 (p2p_est_pose_opts.det_mask given; tools/5_evaluation_bop_basic.py:307-316): {intersection, union,
                           * valid_mask pixel count} of the detector mask with valid_mask_full -- the same numbers opts.mask_stats receives,
                           * carried in the record so that a GATHERED record (p2p_est_pose_collect_gathered) is all another rank needs to
                           * score the detection; zeros otherwise */
} p2p_pose;

/* Optional knobs; zero-initialise for the reference behaviour. */
typedef struct {
    /* PnP-RANSAC constants hard-coded at recognition.py:216-217 / OpenCV defaults. 0 => default */
    int ransac_iterations;      /* 100; at most P2P_MAX_RANSAC_ITERATIONS */
    double reprojection_error;  /* 5.0  */
    double confidence;          /* 0.99 */
    /* TEST / BENCH ONLY: replace the decoder outputs after each generator pass (device
     * pointers).  inject1: [n_det,128,128,4]; inject2: [n_det,n_outlier_th_max,128,128,4].
     * The generator still runs (and is timed); its output is then overwritten.  No trained
     * weights exist offline, so synthetic scenes drive the PnP stage this way. */
    const float* inject1;
    const float* inject2;
    int inject_slots;           /* second dimension of inject2 */
    /* optional per-detection outputs, host pointers (may be null):
     * valid_mask [n_det][mask_stride] bytes (H*W of the detection's frame used),
     * img_pred   [n_det][pred_stride] bytes (crop h*w*3 used) */
    unsigned char* valid_mask;
    int64_t mask_stride;
    unsigned char* img_pred;
    int64_t pred_stride;
    /* optional debug taps (host pointers, may be null): stage-1 inputs [n_det,128,128,3] and
     * stage-2 inputs [n_det,K,128,128,3], K = max n_outlier_th over the objects in the batch */
    float* dbg_x1;
    float* dbg_x2;
    int* dbg_boxes2;            /* [n_det][12] stage-2 get_boxes result */
    int* dbg_cand;              /* [n_det][K][6]: valid, n_non_gray, n_corr, n_inliers, ransac iters, best iter */
    /* the generator's raw answers (x, y, z, prob) of both stages: [n_det,128,128,4] and [n_det,K,128,128,4] (slot k of a detection = its
     * k-th outlier threshold; slots without a stage-2 input hold garbage).  The shim builds the reference's FAILURE returns from them: the
     * first tuple element of recognition.py:127 / :191 is the stage-1 / last candidate's clipped (decode + 1) / 2 preview. */
    float* dbg_y1;
    float* dbg_y2;
    /* score_type 2 support (reference tools/5_evaluation_bop_basic.py:307-316): per-detection
     * detector masks, host pointer [n_det][det_mask_stride] bytes (non-zero = object), same H x W
     * as the detection's frame; mask_stats (host, [n_det][3]) receives
     * {intersection, union, valid_mask pixel count} of the detector mask with valid_mask_full. */
    const unsigned char* det_mask;
    int64_t det_mask_stride;
    int64_t* mask_stats;
    /* skimage.transform.resize GENERATION switch.  The reference calls resize(order=1) six times per detection
     * (recognition.py:82,103,121,134,144,146) and does not pin scikit-image (requirements.txt does not list it):
     * Values outside 0 .. 2 are refused (P2P_ERR_INVALID_ARG).
     *   0 (default): scikit-image <= 0.14 -- plain bilinear warp, every image warped in double (the 0.14 _warp_fast takes doubles only).
     *      PINNED to the real library's float64 warp: no 0.14 wheel exists in the build image, but what 0.14 runs for order=1 -- _warp_fast in
     *      double, the reflect / constant border modes, clip -- is what the real 0.18.3 runs for resize(image.astype(float64),
     *      anti_aliasing=False); tests/golden/reference_est_pose_skimage014.json is the reference's est_pose with that on all six call
     *      sites (masks, uint8 images, boxes, poses identical).  Restated: that 0.14 converts every image to double before the warp.
     *   1: scikit-image 0.17 - 0.18, PINNED bit for bit to the real 0.18.3 (+ scipy 1.7.1) of the build image's /opt/conda/bin/python3.9
     *      (tests/golden/external_vectors.json: resize itself; tests/golden/reference_est_pose_skimage018.json: the reference's est_pose
     *      with the real library on all six call sites -- masks, uint8 images, boxes identical):
     *      - anti_aliasing is on by default for float images: every DOWN-scaling resize of one is preceded by
     *        scipy.ndimage.gaussian_filter(sigma = (in/out - 1)/2, truncate 4, border 'mirror' / 'constant'+cval, result kept in the
     *        array's dtype), restated in csrc/resize_aa.hip -- and off for BOOL images (the keep mask of recognition.py:103);
     *      - warp() keeps a FLOAT32 image float32: the prob map of :134 and img_pred of :144 are interpolated by
     *        _warp_fast[float32] (matrix, source coordinates and taps in float32, the blend as the 0.18.3 wheel compiles it), the
     *        result is compared with th_inlier in float32 (:203) and multiplied by 255 in float32 (:144) before the uint8 truncation.
     *      One thing of the real library is NOT reproduced because it is not reproducible: resize() fits its scale-and-shift matrix by SVD,
     *      and the fit's 1e-14 noise -- which depends on the BLAS kernels the machine selects -- decides `> 0.9` on mask pixels whose
     *      bilinear weight is exactly 0.9 (crop sides that are multiples of 10).  This library uses the exact map the fit approximates;
     *      the fixture records both and shows the same wheels disagreeing with themselves across OPENBLAS_CORETYPE settings.
     *   2: scikit-image 0.15 / 0.16 -- what the reference's OWN image resolves to (requirements.txt:7 imgaug==0.2.7 pulls scikit-image,
     *      Dockerfile:1,5 is python 3.5, which caps it at 0.15.x).  anti_aliasing defaults to True for EVERY image: resize() hands the image
     *      as passed to scipy.ndimage.gaussian_filter, so the float32 maps are filtered in float32 as in generation 1 -- and the BOOL keep mask
     *      of recognition.py:103 is filtered into a BOOL array (each axis pass ends in a cast to npy_bool: a pixel survives only where its
     *      weighted sum reaches 1.0; depending on how the weights' sum rounds for the crop side, part of the mask survives or none of it);
     *      warp() then converts every image to double (the 0.15 / 0.16 _warp_fast takes doubles only), so interpolation, the th_inlier
     *      comparison and the * 255 are in double as in generation 0.  PINNING: no 0.15 wheel exists in the build image; the fixture
     *      (tests/golden/reference_est_pose_skimage015.json) runs the reference's est_pose with resize COMPOSED of the real scipy 1.7.1 filter on
     *      the image as passed and the real scikit-image 0.18.3 float64 warp -- filter (bool path included) and warp pinned, their order and the
     *      double conversion restated from the 0.15 / 0.16 sources.  The Gaussian weights are built with libm's exp like numpy <= 1.18 (the
     *      reference's era); numpy >= 1.19 uses a SIMD exp 1 ulp apart on some arguments, which the bool filter can amplify into a whole mask.
     *      So against a caller's scipy this generation is bit-exact only for crop sides whose weights agree between the two exp
     *      implementations (the parity tests skip the others; p2p_aa_weights() returns the library's weights of a side for comparison).
     * (scikit-image >= 0.19 rejects the bool array of recognition.py:103, so the reference does not run there.)
     * clip=True of resize (output clamped to the input's range, cval preserved) is common to all versions and always on. */
    int resize_anti_aliasing;
    /* p2p_est_pose_submit only: let the NEXT submit run this batch's stage-2 generator pass merged with its own stage-1
     * pass (one pass over [x2(k) | x1(k+1)] when the newcomer is not larger; collect runs it alone otherwise).  Fewer, larger
     * passes -- pays for small batches; at 256 detections per batch the chip is full either way (measured equal), so the
     * default is off.  Results are identical. */
    int merge_stream_passes;
    /* The valid_mask buffers are zero-filled already (freshly calloc'ed pages, numpy.zeros): the library then writes only the rows of
     * each detection's crop instead of clearing H x W bytes per detection first (256 detections of 640 x 480 frames: 79 MB of page
     * touching per batch on the calling thread).  0 = the library clears them (valid_mask_full = zeros, recognition.py:175).
     * PRECONDITION, not checked: with 1 the buffer must be all-zero before EVERY call that names it -- the library writes the crop rows
     * of detections with status OK and nothing else, so a buffer reused across calls (the natural pattern with submit / collect) keeps
     * the previous batch's rows, and the rows of detections that fail this time.  Re-zero it, allocate a fresh one, or pass 0. */
    int mask_prezeroed;
} p2p_est_pose_opts;

/* Blocking.  poses[i] corresponds to dets[i]. */
P2P_API int p2p_est_pose_batch(p2p_ctx* ctx, const p2p_object* objects, int n_objects, const p2p_image* images,
                       int n_images, const p2p_detection* dets, int n_dets, p2p_pose* poses,
                       const p2p_est_pose_opts* opts);

/* Asynchronous form of p2p_est_pose_batch for detection streams: `submit` only enqueues the batch
 * (generator passes + glue on the context stream, PnP-RANSAC + selection + D2H on a second stream)
 * and returns a ticket; `collect` waits for that batch and fills poses[n_dets].  At most two
 * batches may be in flight, so the latency-bound PnP tail of batch i overlaps the generator
 * passes of batch i+1.  Device-resident frames and injected maps must stay alive until the
 * collect.  The optional outputs of the reference's return tuple (valid_mask, img_pred: recognition.py:189-193)
 * and the score_type-2 sums (det_mask -> mask_stats) are available here too: name the host buffers in the
 * options of `submit`, keep them alive, and `collect` fills them (rendered on the tail stream, landed in pinned
 * memory, copied out at collect time).  det_mask is read during `submit`.  Only the debug taps are blocking-only. */
P2P_API int p2p_est_pose_submit(p2p_ctx* ctx, const p2p_object* objects, int n_objects, const p2p_image* images,
                        int n_images, const p2p_detection* dets, int n_dets, const p2p_est_pose_opts* opts,
                        int* ticket);
P2P_API int p2p_est_pose_collect(p2p_ctx* ctx, int ticket, p2p_pose* poses);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU (no reference call site -- tools/5_evaluation_bop_basic.py:289-304 walks the detections of an
 * image one by one on one GPU).  Detections are independent: one process per GPU, each with its own p2p_ctx, runs the whole
 * pipeline on its shard.  The only exchange is one RCCL all-gather (xGMI) of the final p2p_pose records per batch.
 *   p2p_comm_unique_id   rank 0 draws the 128-byte id; the host program hands it to the other ranks by whatever it has
 *                        (MPI, a file, torch.distributed, a socket).
 *   p2p_comm_create      every rank: joins the communicator on its context's device (ncclCommInitRank -- collective).
 *   p2p_est_pose_collect_gathered   p2p_est_pose_collect + the gather: once the batch's tail has finished, its records go DEVICE to DEVICE over
 *                        the communicator (they never visit the host first) and are copied out once.
 *                        `poses[n_dets]` = this rank's own results as from collect; `gathered[world][n_max]` = every rank's records in
 *                        its caller's detection order, padded with status = P2P_POSE_ABSENT.  n_max >= the largest batch of any rank
 *                        and equal on all ranks.  Collective: every rank calls it once per step, in the same order.
 *                        A rank WITHOUT work this step (an empty shard: images run out on different ranks, an object group smaller than
 *                        the world -- the ragged loop of tools/5_evaluation_bop_basic.py:289-304) calls it with ticket = P2P_TICKET_NONE
 *                        (poses may be NULL) and contributes n_max padding records; p2p_est_pose_submit itself takes n_dets >= 1.
 *                        Errors never strand the peers: once ctx / comm / gathered / n_max are sane the all-gather is entered on every
 *                        path -- an unknown ticket, a batch larger than n_max (its ticket stays in flight for a plain collect) or a failed
 *                        stage-2 flush contribute padding and are returned AFTER the collective.  A batch that left the split-f16 operand
 *                        range (P2P_ERR_RANGE on this rank, nothing handed over) travels as P2P_POSE_RANGE records.
 * RCCL is bound at run time (an RCCL already mapped into the process -- PyTorch's wheel carries one -- is reused, else librccl.so.1;
 * P2P_RCCL_LIB overrides): the library loads and runs single-GPU on machines without RCCL; these calls then fail with P2P_ERR_HIP.
 * ---------------------------------------------------------------------------------------- */
#define P2P_COMM_ID_BYTES 128
#define P2P_TICKET_NONE (-1)
typedef struct p2p_comm p2p_comm;
P2P_API int p2p_comm_unique_id(char* id /* [P2P_COMM_ID_BYTES] */);
P2P_API int p2p_comm_create(p2p_ctx* ctx, int rank, int world, const char* id /* [P2P_COMM_ID_BYTES] */, p2p_comm** out);
P2P_API void p2p_comm_destroy(p2p_comm* comm);
P2P_API const char* p2p_comm_library(void);   /* path of the RCCL the calls above bound ("" if none could be) */
P2P_API int p2p_est_pose_collect_gathered(p2p_ctx* ctx, p2p_comm* comm, int ticket, p2p_pose* poses, int n_max, p2p_pose* gathered);

/* Replaces `cv2.solvePnPRansac(obj, img, camK, None, flags=EPNP, reprojectionError, iterationsCount)`
 * + `cv2.Rodrigues` (reference recognition.py:216-223) for a batch of independent problems.
 * Problem p owns points [offsets[p], offsets[p+1]) of obj_pts [N,3] (mm, double) and img_pts
 * [N,2] (pixels, double); camK [n_problems][9].  Host pointers.  ok[p]=0 reproduces cv2 returning
 * inliers=None.  inlier_mask (may be null) is [N] bytes.  info[p] = {n_inliers, iterations, best_iter}. */
P2P_API int p2p_pnp_ransac_batch(p2p_ctx* ctx, const double* camK, const double* obj_pts, const double* img_pts,
                         const int* offsets, int n_problems, int iterations, double reprojection_error,
                         double confidence, double* R, double* t, int* info, int* ok,
                         unsigned char* inlier_mask);

/* ------------------------------------------------------------------------------------------
 * Measurement hooks (bench.py): when enabled, every launch of a convolution kernel of the generator is
 * bracketed by HIP events on the stream it is launched on; stats are per kernel family:
 *   0  igemm_kernel 128x128 tiles     1  igemm_kernel 128x64 tiles     2  igemm_kernel 128x32 tiles
 *   3  igemm_halo_kernel<2,2> (halo-tiled stride-1 multi-tap layers, 128x128 tiles)     4  igemm_halo_kernel<4,2> (Cout = 64 layers, 256x64 tiles)
 *   5  heads_halo_kernel (merged output heads)     6  igemm_halo8_kernel (layers on the 8x8 grid: conv4, first transposed conv)
 *   7  igemm_halo_s2_kernel (5x5 stride-2 convolutions on larger grids: the paper encoder's conv2 / conv3)
 *   8  igemm_stream_kernel (small launches: one wave per 32x32 tile, same K order and bits as the batched kernels)
 *   9  resblock_kernel (a ResNet identity bottleneck block -- 1x1, 3x3, 1x1 + residual -- in one launch, intermediates in LDS)
 *   10 wino_gemm_kernel (the 5x5 stride-1 decoder layers in Winograd F(4,5) form along the row axis: 2.5x fewer MFMA products; algo_flops
 *      stays the DIRECT form's 2 x MACs of the layer)     11 wino_input_kernel (its input transform: x -> split-f16 V in HBM; algo_flops 0)
 *   12..19 the bandwidth- / latency-leaning kernels around the generator, time and launches only (their work depends on device-side counts:
 *      bench.py prices them on the batch's correspondence / pixel counts):  12 pnp_hypotheses_kernel   13 pnp_count_kernel   14 pnp_score_kernel
 *      15 pnp_fit_solve_kernel + pnp_fit_select_kernel   16 aa_filter_kernel<0>   17 aa_filter_kernel<1>
 *      18 cand_eval_kernel + cand_compact_kernel (or cand_corr_kernel)   19 stage2_input_kernel
 *   20 wino3_gemm_kernel (the transposed convolutions up2 / up3 in Winograd F(4,3) form along the row axis: 15 position-products per input
 *      pixel instead of 25; algo_flops = the DIRECT form's 2 x MACs)     21 wino3_input_kernel (its input transform; algo_flops 0)
 * algo_flops counts the layers' algorithmic FLOPs (2 x MACs of the reference layer, SURVEY.md
 * section 8a-L), not padded work and not the 3 MFMA products per MAC of the split-f16 arithmetic.
 * ---------------------------------------------------------------------------------------- */
#define P2P_PROFILE_SLOTS 22
typedef struct {
    int64_t launches;
    double total_ms;
    double algo_flops;
    double algo_bytes;   /* compulsory HBM bytes of the launches: the layer's input tensor(s) + residual + weights read once, its output
                          * written once, fp32 -- what an HBM roofline of the bandwidth-leaning kernels is priced on */
} p2p_kernel_stats;

P2P_API int p2p_profile_enable(p2p_ctx* ctx, int on);
/* Harvest finished events (synchronises the stream) and return the accumulated stats; reset
 * clears the accumulators afterwards.  stats must hold P2P_PROFILE_SLOTS entries. */
P2P_API int p2p_profile_read(p2p_ctx* ctx, p2p_kernel_stats* stats, int reset);

/* ------------------------------------------------------------------------------------------
 * Depth path (RGB-D scoring, reference tools/5_evaluation_bop_icp3d.py).  csrc/depth.hip; DESIGN.md section 8.
 * ---------------------------------------------------------------------------------------- */
typedef struct p2p_mesh p2p_mesh;   /* one object's triangle mesh, vertices in HBM */

/* Upload a mesh (reference: rendering/model.py Model3D.load, and pix2pose_amd/mesh.py read_ply): verts_mm [n_verts][3] in mm
 * (the library stores them in metres, like Model3D.load(scale=0.001)), tris [n_tris][3] vertex indices (host pointers).  An index
 * outside [0, n_verts) is P2P_ERR_INVALID_ARG. */
P2P_API int p2p_mesh_create(p2p_ctx* ctx, const float* verts_mm, int n_verts, const int* tris, int n_tris, p2p_mesh** out);
P2P_API void p2p_mesh_destroy(p2p_mesh* mesh);

/* One detection of the depth path, in the units of p2p_pose: mesh meshes[mesh_idx] at pose (R, t) through camK, t in mm.  The
 * library hands t/1000 to the rasteriser like icp3d.py passes tra_pred/1000 to render_obj(), and keeps render_obj's unit quirk on
 * that value (:46: tra[2] > 100 m is taken as mm and divided by 1000 once more).  img_idx indexes the depth images of
 * p2p_depth_score_batch (ignored by p2p_render_depth_batch); union_mask is a host u8 [height*width] (nonzero = in the union mask,
 * p2p_depth_score_batch, p2p_icp_inputs_batch and p2p_refine_depth_batch).  It is also the job record of the depth refinement entry
 * point p2p_refine_depth_batch. */
typedef struct {
    int img_idx;
    int mesh_idx;
    double camK[9];
    double R[9];
    double t[3];
    const unsigned char* union_mask;
} p2p_refine_job;

/* Depth-only z-buffer (replaces render_obj(), icp3d.py:40-50, and rendering/renderer_xyz.py Renderer): depth [n_jobs][height][width]
 * float32 in metres, 0 where nothing is drawn (host pointer).  Nearest surface, coverage at pixel centres (u, v) = (i + 0.5, j + 0.5),
 * 1/z interpolated in screen space, near / far clip 0.01 / 10 m, back faces culled; the coverage rule is in DESIGN.md section 8.
 * Deterministic: the result does not depend on triangle order or on the other jobs of the batch. */
P2P_API int p2p_render_depth_batch(p2p_ctx* ctx, const p2p_mesh* const* meshes, int n_meshes, const p2p_refine_job* jobs, int n_jobs,
                                   int height, int width, float* depth);

/* Depth agreement of a detection (icp3d.py:470-490, fcn() at :314-315): renders job j as above and compares it with the sensor depth
 * depth_images[job.img_idx] (host float32 [height][width], metres: the caller applies depth_scale, icp3d.py:360) over the union mask:
 * diff = |depth_ref - depth_t|, inlier_count = sum(diff < 0.02), fcn = sum(max(0, 0.02 - diff)) / 0.02, ratio = inlier_count / union.
 * inlier_masks (may be null): host u8 [n_jobs][height][width], 1 where in the union mask and diff < 0.02.  fcn is summed in a fixed
 * order, so a job's score is bit-identical alone or in a batch.  The caller forms the score (det_score * fcn in the first round). */
typedef struct {
    int64_t inlier_count;
    int64_t union_count;
    double fcn;
    double ratio;        /* inlier_count / union_count (0 when the union is empty) */
} p2p_depth_score;

P2P_API int p2p_depth_score_batch(p2p_ctx* ctx, const p2p_mesh* const* meshes, int n_meshes, const float* const* depth_images,
                                  int n_images, const p2p_refine_job* jobs, int n_jobs, int height, int width, p2p_depth_score* out,
                                  unsigned char* inlier_masks);

/* ------------------------------------------------------------------------------------------
 * Depth back-projection, normals and the ICP point sets (csrc/normals.hip).  A point is 6 float32
 * [x y z nx ny nz], xyz in the depth's unit (metres).  Normals follow get_normal(refine=True) with cv2.inpaint replaced by the
 * onion-peel fill of DESIGN.md 8 (outputs at pixels with d > 0 do not depend on the fill's depth); pixel offsets are the reference's
 * int16 (u - cx), (v - cy), truncated toward zero, and the skew camK[1] is not used.  Image sizes from 3 x 3 to 16384 x 16384
 * (at most 2^26 pixels), cameras with finite nonzero fx, fy and |cx|, |cy| < 16384; anything else is P2P_ERR_INVALID_ARG.
 * ---------------------------------------------------------------------------------------- */

/* Scene points of whole frames (replaces getXYZ + get_normal(refine=True) at icp3d.py:372-374): depth_images[i] host float32
 * [height][width] in metres, camK [n_images][9] (row-major 3 x 3), points host float32 [n_images][height][width][6]. */
P2P_API int p2p_depth_points_batch(p2p_ctx* ctx, const float* const* depth_images, int n_images, const double* camK, int height,
                                   int width, float* points);

/* Status of an ICP input record.  Both nonzero values are the reference's `return tf, -1` (icp_refinement :70-73). */
enum {
    P2P_ICP_OK = 0,
    P2P_ICP_SMALL_BBOX = -1,      /* bbox of init_mask: rmax - rmin < 5 or cmax - cmin < 5 (also an empty init_mask) */
    P2P_ICP_FEW_POINTS = -2,      /* fewer than 10 init_mask pixels in the whole image */
    P2P_ICP_NONFINITE = -3        /* p2p_icp_batch / p2p_refine_depth_batch only: a source or target xyz is not finite (a NaN sensor
                                   * pixel inside the union mask), or the normalisation scale is not (every point at the mean);
                                   * p2p_icp_inputs_batch never returns it */
};

/* One job's ICP inputs.  Offsets and counts are in points, into the packed buffers of p2p_icp_inputs_batch.  bbox is
 * get_bbox_from_mask(init_mask) = [rmin, cmin, rmax, cmax], max inclusive (zeros for an empty mask).  t_init: job.t after the
 * 300 / 5000 mm replacement (t := centroid_tgt * 1000), the pose that is rendered; t_adjusted = t_init + (centroid_tgt - centroid_src)
 * * 1000 (mm).  Centroids are float64 means of the stored float32 xyz (before the shift of the source points); an empty set gives NaN.
 * When status != 0: n_src = 0, centroid_src = 0 and t_adjusted = t_init. */
typedef struct {
    int status;
    int bbox[4];
    int64_t src_offset, n_src, tgt_offset, n_tgt;
    double t_init[3], t_adjusted[3], centroid_src[3], centroid_tgt[3];
} p2p_icp_input;

/* The point sets icp_refinement hands to cv2.ppf_match_3d_ICP (icp3d.py:464 and icp_refinement :58-85, up to registerModelToScene):
 *   target: points_tgt[union_mask], the scene points of depth_images[job.img_idx] (computed once per image and camera in a call);
 *   source: at t_init, the render's init_mask = (depth > 0) & union_mask, its bbox and gates, then the points with normals of the
 *           rendered depth over [rmin, rmax) x [cmin, cmax) where init_mask is set, xyz shifted by centroid_tgt - centroid_src.
 * job.union_mask is used as given (the caller ANDs in depth_valid, icp3d.py:455-456).  Points are in numpy's boolean-index (row-major)
 * order, packed in job order into src_points [src_capacity][6] and tgt_points [tgt_capacity][6] (host float32).  A null buffer is
 * not written (records only).  A buffer too small for its points gives P2P_ERR_CAPACITY with every record filled in and no points
 * written, so the caller can size the buffers and call again.  Bit-identical for a job alone or in a batch. */
P2P_API int p2p_icp_inputs_batch(p2p_ctx* ctx, const p2p_mesh* const* meshes, int n_meshes, const float* const* depth_images,
                                 int n_images, const p2p_refine_job* jobs, int n_jobs, int height, int width, p2p_icp_input* out,
                                 float* src_points, int64_t src_capacity, float* tgt_points, int64_t tgt_capacity);

/* ------------------------------------------------------------------------------------------
 * Point-to-plane ICP and the depth refinement entry point (csrc/icp.hip).  The ICP is a named, deterministic
 * restatement of cv::ppf_match_3d::ICP::registerModelToScene (opencv-contrib 3.4.2, the reference's pin): its rules are written down
 * in DESIGN.md 8.2 and held by tests/icp_ref.py; it is not pinned to the OpenCV binary.  A job's result is bit-identical alone or in a
 * batch.
 * ---------------------------------------------------------------------------------------- */
#define P2P_ICP_MAX_LEVELS 8
/* cv2.ppf_match_3d_ICP(iterations, tolerence, rejectionScale, numLevels); a null pointer means the reference's 100, 0.005, 2.5, 2.
 * num_levels outside 1..8, max_iterations < 1, or a non-finite tolerance / rejection_scale is P2P_ERR_INVALID_ARG.  rejection_scale
 * <= 0 turns the robust rejection off (every pair is kept), as in OpenCV. */
typedef struct {
    int max_iterations;
    float tolerance;
    float rejection_scale;
    int num_levels;
} p2p_icp_params;

typedef struct {
    int status;                              /* 0, P2P_ICP_SMALL_BBOX, P2P_ICP_FEW_POINTS (passed through) or P2P_ICP_NONFINITE */
    int iterations[P2P_ICP_MAX_LEVELS];      /* iterations run per pyramid level, index = level (0 = finest) */
    int pairs[P2P_ICP_MAX_LEVELS];           /* selInd of the level's last iteration (0: no iteration) */
    double fval_min[P2P_ICP_MAX_LEVELS];     /* least residual of the level (9999999999 when it ran no iteration); diagnostic */
    double scale, mean_avg[3];               /* the normalisation: xyz -> (xyz - mean_avg) * scale */
    double pose[16];                         /* row-major 4 x 4, metres: registerModelToScene's pose (identity when status != 0) */
} p2p_icp_result;

/* ICP of packed point sets as p2p_icp_inputs_batch returns them: job k registers src_points[inputs[k].src_offset ..][6] (n_src rows)
 * to tgt_points[inputs[k].tgt_offset ..][6] (n_tgt rows), host float32.  Records with status != 0 are passed through with an
 * identity pose.  A job of status 0 with no target point, or whose source is too small for the pyramid (rint(n_src / 2^(levels-1))
 * = 0), is P2P_ERR_INVALID_ARG. */
P2P_API int p2p_icp_batch(p2p_ctx* ctx, const p2p_icp_input* inputs, int n_jobs, const float* src_points, const float* tgt_points,
                          const p2p_icp_params* params, p2p_icp_result* out);

/* The depth refinement of one frame's detections (icp3d.py:455-491): per job, the ICP inputs of p2p_icp_inputs_batch, the ICP above
 * on them without leaving the device, the refined pose tf = icp.pose * [job.R | input.t_adjusted / 1000] (R = tf[:3,:3], t =
 * tf[:3,3] * 1000 mm), and the depth score of p2p_depth_score_batch at (R, t) against the same image and union mask.  A job whose
 * status is not 0 keeps job.R / job.t, an identity icp.pose and a zero score (its inlier mask is all 0).  inlier_masks as in
 * p2p_depth_score_batch (may be null).  The parameter checks of p2p_icp_batch hold per call: a status-0 job whose source is too small
 * for params->num_levels (rint(n_src / 2^(levels-1)) = 0) fails the whole call with P2P_ERR_INVALID_ARG, and n_src is only known
 * inside the call.  With at most 5 levels this cannot happen (a status-0 job has at least 10 source points). */
typedef struct {
    p2p_icp_input input;
    p2p_icp_result icp;
    double R[9];
    double t[3];
    p2p_depth_score score;
} p2p_refine_result;

P2P_API int p2p_refine_depth_batch(p2p_ctx* ctx, const p2p_mesh* const* meshes, int n_meshes, const float* const* depth_images,
                                   int n_images, const p2p_refine_job* jobs, int n_jobs, int height, int width,
                                   const p2p_icp_params* params, p2p_refine_result* out, unsigned char* inlier_masks);

/* ------------------------------------------------------------------------------------------
 * RGB-D evaluation of an image chunk (csrc/rgbd.hip): the per-image loop of tools/5_evaluation_bop_icp3d.py
 * :331-540 with its frames, detector masks, inlier masks and occupancy images kept on the device.  A handle holds one chunk.
 * ---------------------------------------------------------------------------------------- */
typedef struct p2p_rgbd p2p_rgbd;

typedef enum { P2P_DEPTH_U16 = 0, P2P_DEPTH_F32 = 1 } p2p_depth_dtype;

/* Status of a refine record of p2p_rgbd_refine whose union det_mask & depth_valid has 30 pixels or fewer (icp3d.py:457-460): the job
 * is not refined; its record keeps job.R / job.t, an identity icp.pose, a zero score and an all-zero inlier mask. */
#define P2P_RGBD_SMALL_UNION (-4)

/* Candidate codes of p2p_rgbd_resolve (cand_ref < 0) */
#define P2P_RGBD_NOT_EVALUATED (-1)   /* not in the evaluated superset: the walk reaching it is an error (P2P_ERR_INVALID_ARG) */
#define P2P_RGBD_EST_FAILED (-2)      /* est_pose status != 0 (frac_inlier == -1, :444-445) */
#define P2P_RGBD_NEAR (-3)            /* est_pose t[2] / 1000 < 0.2 (:449-450) */

P2P_API int p2p_rgbd_create(p2p_ctx* ctx, p2p_rgbd** out);
/* Does not use the context: a handle may be destroyed after the context it was created on. */
P2P_API void p2p_rgbd_destroy(p2p_rgbd* h);

/* Load a chunk of n_images frames of height x width (replaces the chunk held before).  rgb[i]: host u8 [H][W][3] (gray frames
 * replicated to three channels by the caller); depth[i]: host u16 or float32 [H][W] (depth_dtype) in the sensor's unit; depth_scale[i]
 * from scene_camera.json.  On the device, per pixel and all in float32 without contraction (:360-370):
 *   depth_t = (raw / 1000) * depth_scale,  depth_valid = depth_t > 0.2f && depth_t < 2.2f,
 *   rgb_valid = depth_valid || nan_to_num(depth_t) == 0,  frame = rgb_valid ? float(rgb) : float(rgb) * 0.1f.
 * masks: host u8 [n_masks][H][W] (nonzero = in), the detector masks of the chunk; mask_image[m] names the frame of mask m. */
P2P_API int p2p_rgbd_load(p2p_rgbd* h, const unsigned char* const* rgb, const void* const* depth, int depth_dtype,
                          const double* depth_scale, int n_images, int height, int width, const unsigned char* masks,
                          const int* mask_image, int n_masks);
/* The device frame i of the loaded chunk as a P2P_MEM_DEVICE, P2P_IMG_F32 p2p_image for p2p_est_pose_batch / _submit; valid until the
 * next load or destroy. */
P2P_API int p2p_rgbd_image(p2p_rgbd* h, int i, p2p_image* out);
/* Copies of frame i's depth_t [H][W], depth_valid [H][W] (0 / 1) and frame [H][W][3] (host; each may be null). */
P2P_API int p2p_rgbd_read(p2p_rgbd* h, int i, float* depth_t, unsigned char* depth_valid, float* frame);

/* The depth refinement of p2p_refine_depth_batch with its inputs on the device: job k refines against depth_t of frame jobs[k].img_idx
 * over the union mask det_mask[mask_idx[k]] & depth_valid (jobs[k].union_mask is ignored).  union_counts [n_jobs] (host) receives each
 * union's pixel count; a union of 30 or fewer pixels gets a P2P_RGBD_SMALL_UNION record and is not refined.  Every other record and its
 * inlier mask equal p2p_refine_depth_batch's on the same inputs bit for bit.  The records and inlier masks stay in the handle for
 * p2p_rgbd_resolve (until the next refine or load); inlier_masks (host u8 [n_jobs][H][W], may be null) receives a copy.  A mask
 * index outside the loaded masks, or one of another frame than the job's, is P2P_ERR_INVALID_ARG. */
P2P_API int p2p_rgbd_refine(p2p_rgbd* h, const p2p_mesh* const* meshes, int n_meshes, const p2p_refine_job* jobs, const int* mask_idx,
                            int n_jobs, const p2p_icp_params* params, p2p_refine_result* out, int64_t* union_counts,
                            unsigned char* inlier_masks);

/* One round (0 or 1) of the per-image walk (:394-510), one workgroup per image, occupancy images on the device (round 0 clears them).
 *   images:     tgt_off [n_images + 1] into target_obj / inst_count (the image's targets, in order); roi_off [n_images + 1] into the rois.
 *   rois:       roi_obj, roi_score (detector score), roi_valid (0 for a (-1, -1) roi), roi_mask (detector mask index of the loaded chunk);
 *               cand_off [n_rois + 1] into the candidates of each roi.
 *   candidates: cand_obj (object id) and cand_ref: the index of its refine record, or P2P_RGBD_NOT_EVALUATED / _EST_FAILED / _NEAR.
 *   records:    those of the last p2p_rgbd_refine, or when host_records is not null, host_records [n_records] with host_masks
 *               [n_records][H][W] (host u8, may be null: all-zero inlier masks).
 * In / out: roi_used [n_rois] (0 / 1) and inst_pred [total targets] (the reference's roi_used and inst_count_pred; round 0 starts them
 * at 0).  Out: rows [n_rois][16] = obj_id (0: no row), score, R[9], t[3] (mm), round, r_id -- a roi appends at most one row a round,
 * so the rows of an image in roi order are its result list in append order.  A walk that reaches a NOT_EVALUATED candidate is
 * P2P_ERR_INVALID_ARG. */
P2P_API int p2p_rgbd_resolve(p2p_rgbd* h, int round, int n_images, const int* tgt_off, const int* target_obj, const int* inst_count,
                             const int* roi_off, const int* roi_obj, const double* roi_score, const int* roi_valid, const int* roi_mask,
                             const int* cand_off, const int* cand_obj, const int* cand_ref, const p2p_refine_result* host_records,
                             const unsigned char* host_masks, int n_records, int* roi_used, int* inst_pred, double* rows);

/* ------------------------------------------------------------------------------------------
 * XYZ-coloured renders (training targets, reference tools/2_2_render_pix2pose_training.py through rendering/renderer_xyz.py).
 * csrc/depth.hip; DESIGN.md section 8.4.
 * ---------------------------------------------------------------------------------------- */

/* Per-vertex colours of a mesh: rgb host u8 [n_verts][3] (the red, green, blue properties of a models_xyz PLY), stored as
 * float32(c) / 255 like Model3D.load.  n_verts must equal the mesh's vertex count.  May be called again to replace the colours. */
P2P_API int p2p_mesh_set_colors(p2p_mesh* mesh, const unsigned char* rgb, int n_verts);

/* Colour z-buffer of the jobs of p2p_render_depth_batch (union_mask and img_idx unused): geometry, coverage, clipping and the depth
 * value are that entry point's, bit for bit.  color: host float32 [n_jobs][height][width][3], channel order (x, y, z) = the PLY's
 * (red, green, blue); the perspective-correct varying c = (sum b_i c_i / z_i) / (sum b_i / z_i) of the fragment that owns the pixel,
 * fp64 without contraction, stored as float32; 0 where nothing is drawn.  The owner is the nearest fragment; among fragments of equal
 * float32 depth the lowest triangle index (GL_LESS, triangles drawn in index order).  depth (may be null): host float32
 * [n_jobs][height][width].  bbox (may be null): host int [n_jobs][4] = [min v, min u, max v, max u] of depth > 0, max inclusive
 * (get_rendering's box), reduced on the device; [-1, -1, -1, -1] for an empty render.  A job's result is bit-identical alone or in
 * a batch and from call to call.  A mesh without colours is P2P_ERR_INVALID_ARG. */
P2P_API int p2p_render_xyz_batch(p2p_ctx* ctx, const p2p_mesh* const* meshes, int n_meshes, const p2p_refine_job* jobs, int n_jobs,
                                 int height, int width, float* color, float* depth, int* bbox);

/* Training patches from colour renders (tools/2_2_render_pix2pose_training.py:168-184).  Job k: rgb[k] host u8 [height][width][3],
 * its render color [k][height][width][3] / depth [k][height][width] / bbox [k][4] as p2p_render_xyz_batch returns them (host).  The
 * patch is uint8 [h][w][6]: rgb with [128,128,128] where depth == 0, then xyz -- the colour as the reference reads it back from an
 * 8-bit GL buffer and stores it: q = floor(c * 255 + 0.5), then uint8(float32(float32(q) / 255) * 255), which for some q is q - 1 --
 * cropped to rows bbox[0]:bbox[2], columns bbox[1]:bbox[3] (the box's max is inclusive: the last covered row and column are left
 * out, as in the reference).  When max(h, w) > 128 each half is resized on its own to int(h * s + 0.5) x int(w * s + 0.5),
 * s = 128.0 / max(h, w), by skimage.transform.resize(order = 1) of generation resize_generation (p2p_est_pose_opts.
 * resize_anti_aliasing's numbering: 0, 1 or 2, with that generation's default mode and anti-aliasing) acting on float32(x / 255);
 * the result times 255 is truncated.  patches: host u8 [n_jobs][128][128][6], job k's patch in the
 * top-left shapes[k][0] x shapes[k][1] corner with row stride 128 (the rest 0); shapes: host int [n_jobs][2].  A job whose render is
 * empty (bbox[0] < 0) or whose box has a zero side reports (0, 0) and writes nothing: the caller skips it. */
P2P_API int p2p_xyz_patch_batch(p2p_ctx* ctx, const unsigned char* const* rgb, const float* color, const float* depth, const int* bbox,
                                int n_jobs, int height, int width, int resize_generation, unsigned char* patches, int* shapes);

/* The in-plane rotation copies of those patches (tools/2_2_render_pix2pose_training.py:64-96, augment_inplane_gen with isYCB=False):
 * per job a frame and its render as above (uploaded once per job) and n_angles[k] rotations, each given by what
 * skimage.transform.rotate(resize=True) of scikit-image 0.17 / 0.18 derives from the angle on the host: matrices [item][6] = rows 0 and
 * 1 of the float64 map (x, y, 1) of the rotated image -> (column, row) of the frame, and rot_shapes [item][2] = the rotated frame's
 * (rows, columns); items are the jobs' angles in job order (runtime.xyz_rotate_patch_batch forms both with numpy, so their bits do not
 * depend on the device).  rgb_table / xyz_table: float32 [256], the value the reference's float32 input image holds for the 8-bit
 * level q -- float32(q / 255.0) for the frame (grey 128 where depth == 0), float32(float32(float32(q) / 255) * 255) / 255 for the
 * colour's GL level q = floor(c * 255 + 0.5); entries in [0, 1].  Per item: the box of rotate(depth > 0 as float64) > 0 (fp64 warp,
 * reduced on the device), then per pixel of that box, for both images, the library's float32 warp (cval 0.5 for the frame, 0 for the
 * colour), its clip to the input image's range, times 255 in float32, truncated to uint8; the crop leaves the box's last row and
 * column out; boxes above 128 px are resized like p2p_xyz_patch_batch's.  patches: host u8 [items][128][128][6], shapes: host int
 * [items][2], as above; (0, 0) for an empty render or a box with a zero side.  resize_generation must be 1 (0.17 / 0.18): the other
 * generations hand a float32 image to the warp differently and no real library pins them.  A bad angle list (a negative count, a
 * matrix that is not finite, an impossible shape) is P2P_ERR_INVALID_ARG.  An item's result is bit-identical alone or in a batch. */
P2P_API int p2p_xyz_rotate_patch_batch(p2p_ctx* ctx, const unsigned char* const* rgb, const float* color, const float* depth, int n_jobs,
                                       int height, int width, const int* n_angles, const double* matrices, const int* rot_shapes,
                                       const float* rgb_table, const float* xyz_table, int resize_generation, unsigned char* patches,
                                       int* shapes);

/* ------------------------------------------------------------------------------------------
 * Training batches (reference pix2pose_util/data_io.py:53-274, get_patch_pair).  csrc/train_batch.hip; DESIGN.md section 8.5.
 * ---------------------------------------------------------------------------------------- */

#define P2P_TRAIN_MAX_PATCH 128      /* rows and columns of a train_xyz patch (make_train_xyz's resize rule) */
#define P2P_TRAIN_MAX_WINDOW 250     /* side of the crop window, 2 * int(max(w', h') * 1.5 / 2) with w', h' <= 1.3 * 128 */

/* p2p_train_batch's status per sample */
#define P2P_TRAIN_OK 0
#define P2P_TRAIN_BAD_PATCH (-1)        /* null, not 6 or 7 channels, a side of 0 or above P2P_TRAIN_MAX_PATCH */
#define P2P_TRAIN_BAD_BACKGROUND (-2)   /* null, not 1 or 3 channels, or after the enlargement rule smaller than the patch plus 20 */
#define P2P_TRAIN_BAD_DRAW (-3)         /* a value that is not finite, a paste or window outside the frame, a window above the bound */

/* What one sample's draws of the `random` module come to, every int(...) taken on the host (runtime.train_draws).  The frame is the
 * background after the enlargement rule (:78-85): max(H, 2 h) x max(W, 2 w) where H < 2 h or W < 2 w, else H x W. */
typedef struct p2p_train_draw {
    int v_ref, u_ref;       /* where the patch is pasted (:90-91) */
    int v1, v2, u1, u2;     /* the crop window clipped to the frame (:120-154): rows v1 .. v2, columns u1 .. u2 */
    int side;               /* side of the unclipped window = of base_image (:125) */
    int shift_v, shift_u;   /* shift_v_min, shift_u_min: where the clipped window starts in base_image (:140-150) */
    int rect[3][4];         /* first occlusion (:164), second occlusion (:233), background inclusion (:247): rows r0 .. r1 and columns
                               c0 .. c1 of the frame with Python's slice rule already applied; r0 >= r1 or c0 >= c1: none */
    int even;               /* batch_count % 2 == 0 (:203) */
    int reserved;
    double sigma_edge;      /* :191, the boundary's Gaussian (applied as a dilation) */
    double sigma_blur;      /* :193, the image blur */
    double sigma_ran;       /* :206, clamped to [0.1, 1]; unused when even == 0 */
    double rot[6];          /* rows 0 and 1 of rotate(angle)'s map (x, y, 1) of the output -> (column, row) of base_image (:264-268) */
} p2p_train_draw;

/* Parameters of the colour stage (seq_syn, :42-51) for one sample; see p2p_train_batch.  order: a permutation of 0 .. 7 =
 * Add on channel 0, 1, 2; ContrastNormalization; Multiply; GaussianBlur; AdditiveGaussianNoise; the second ContrastNormalization. */
typedef struct p2p_train_colour {
    int order[8];
    float add[3];
    float contrast;
    float mul[3];
    float blur_sigma;
    float noise_scale;      /* 0: the Sometimes(0.1, ...) did not fire */
    float contrast2[3];     /* 1, 1, 1: the Sometimes(0.5, ...) did not fire */
    unsigned int sample;    /* the noise generator's key is (seed, sample, pixel, channel) */
    unsigned long long seed;
} p2p_train_colour;

/* sizeof of the records above for a binding's self-check: 0 = p2p_train_draw, 1 = p2p_train_colour, else -1 */
P2P_API int p2p_train_sizeof(int which);

/* n training samples in one call: get_patch_pair of scikit-image 0.17 / 0.18 (generation must be 1) from explicit draws.
 * Sample k: patches[k] host u8 [h][w][c] with patch_shapes[k] = (h, w, c), c = 6 or 7 (rgb, xyz, and an unused visibility channel),
 * h, w <= P2P_TRAIN_MAX_PATCH; backgrounds[k] host u8 [H][W][C] with back_shapes[k] = (H, W, C), C = 3 or 1 (grey, replicated);
 * draws[k]; colours[k] when colours is not null (null: the colour stage is skipped, which is the reference with an augmenter that
 * returns its input).  Only the background under the window travels to the device.  Stages as DESIGN.md section 8.5 lists them:
 * enlargement of a small background (float32 warp), compositing, first occlusion, boundary by np.gradient's differences, the two
 * thresholded Gaussians as square dilations of radius int(4 sigma + 0.5), the separable blurs with scipy's weights and
 * mode='nearest', the even-batch branch with its radius > 0.3 test in double, normalisation to [-1, 1], placement, rotation
 * (base and target 'reflect', mask 'constant') and the resize to imsize x imsize (anti-aliased, 'reflect') in double.
 * The colour stage works on the 0 .. 255 float patch, clips to [0, 255] after every augmenter, blurs with mirrored edges, and is a
 * restatement of imgaug's documented meaning, not pinned to it.
 * src, tgt: float32 [n][imsize][imsize][3]; mask: float32 [n][imsize][imsize]; host memory (out_mem = P2P_MEM_HOST) or device
 * memory of the context's device (P2P_MEM_DEVICE); complete when the call returns.  16 <= imsize <= 512.
 * status [n] (host): P2P_TRAIN_OK or the reason the sample was left out (its outputs are 0, p2p_last_error names the first such
 * sample); the other samples are not affected, and a sample's result is bit-identical alone or in a batch.  Returns
 * P2P_ERR_INVALID_ARG only for null arguments, a bad imsize or generation. */
P2P_API int p2p_train_batch(p2p_ctx* ctx, int n, const unsigned char* const* patches, const int* patch_shapes,
                            const unsigned char* const* backgrounds, const int* back_shapes, const p2p_train_draw* draws,
                            const p2p_train_colour* colours, int imsize, int generation, float* src, float* tgt, float* mask, int out_mem,
                            int* status);

#ifdef __cplusplus
}
#endif
#endif /* P2P_MI355_H */
