"""Python handles over the C ABI: a per-GPU context and per-object generator networks."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from . import weights as W


class Context:
    """One GPU's pipeline context (stream + workspaces).  Not thread-safe (p2p_mi355.h)."""

    WINOGRAD = {"off": 0, "auto": 1, "always": 2}

    def __init__(self, device: int = 0, max_batch: int = 256, winograd: str = "auto"):
        self._h = C.c_void_p()
        _lib.check(_lib.lib().p2p_ctx_create(device, max_batch, C.byref(self._h)), "p2p_ctx_create")
        self.device = device
        self.max_batch = max_batch
        if winograd != "auto":
            self.set_winograd(winograd)

    def set_winograd(self, mode: str):
        """Form of the 5x5 layers (deconv1-3, up1-3, conv4) in split-f16 passes (p2p_ctx_set_winograd): "auto" (default) = the fastest form at
        every pass size (Winograd F(4,5) at every size, F(4,3) from 5 / 9 inputs up, K splits for launches that would fill a fraction of the chip) -- a sample's bits depend on the pass SIZE;
        "off" / "always" = one form at every size."""
        _lib.check(_lib.lib().p2p_ctx_set_winograd(self._h, self.WINOGRAD[mode]), "p2p_ctx_set_winograd")

    @property
    def handle(self):
        return self._h

    @property
    def stream(self) -> int:
        return _lib.lib().p2p_ctx_stream(self._h) or 0

    def synchronize(self):
        _lib.check(_lib.lib().p2p_ctx_synchronize(self._h), "p2p_ctx_synchronize")

    def range_event(self) -> float:
        """Largest activation magnitude beyond the split-f16 operand range that direct forward calls (Generator.forward_device) stored since
        the last query; 0.0 = none.  Synchronises the context stream (p2p_ctx_range_event)."""
        v = C.c_float(0.0)
        _lib.check(_lib.lib().p2p_ctx_range_event(self._h, C.byref(v)), "p2p_ctx_range_event")
        return float(v.value)

    def profile(self, on: bool):
        """Bracket every implicit-GEMM launch with HIP events on the context stream."""
        _lib.check(_lib.lib().p2p_profile_enable(self._h, 1 if on else 0), "p2p_profile_enable")

    def profile_read(self, reset=True):
        """-> list of PROFILE_SLOTS dicts (kernel families, see PROFILE_KERNELS): launches, total_ms, algo_flops, algo_bytes."""
        st = (_lib.KernelStats * _lib.PROFILE_SLOTS)()
        _lib.check(_lib.lib().p2p_profile_read(self._h, st, 1 if reset else 0), "p2p_profile_read")
        return [{"launches": int(s.launches), "total_ms": float(s.total_ms), "algo_flops": float(s.algo_flops), "algo_bytes": float(s.algo_bytes)} for s in st]

    def close(self):
        if self._h:
            _lib.lib().p2p_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def default_context(device: int = 0) -> Context:
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


class Generator:
    """Drop-in for the Keras model held in ``pix2pose.generator_train``
    (reference recognition.py:21-26): ``predict(x) -> [decode, prob]`` (recognition.py:84,129)."""

    def __init__(self, weights: dict, backbone: str, ctx: Context | None = None, precision: str = "f16x3"):
        """precision: 'f32' (fp32 matrix instructions), 'f16x3' (fp32 emulated with three split-f16
        MFMAs per product block, fp32 accumulate; see include/p2p_mi355.h) or 'auto' (f16x3 with an fp32 twin the object
        falls back to when an activation leaves the f16 operand range; without a twin such a pass raises P2PRangeError)."""
        if backbone not in _lib.BACKBONE:
            raise ValueError("unknown backbone %r" % (backbone,))
        if precision not in _lib.PRECISION:
            raise ValueError("unknown precision %r" % (precision,))
        self.precision = precision
        W.check_weights(backbone, weights)
        self.ctx = ctx or default_context()
        self.backbone = backbone
        specs = W.tensor_specs(backbone)
        arr = (_lib.Tensor * len(specs))()
        keep = []
        for i, (name, _) in enumerate(specs):
            a = np.ascontiguousarray(weights[name], dtype=np.float32)
            keep.append(a)
            arr[i].name = name.encode()
            arr[i].data = a.ctypes.data_as(C.POINTER(C.c_float))
            arr[i].numel = a.size
        self._h = C.c_void_p()
        _lib.check(_lib.lib().p2p_model_create_ex(self.ctx.handle, arr, len(specs), _lib.BACKBONE[backbone],
                                                  _lib.PRECISION[precision], C.byref(self._h)), "p2p_model_create_ex")

    @property
    def handle(self):
        return self._h

    def predict(self, x):
        """x [N,128,128,3] float (float64 accepted, cast to float32 like Keras does)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 4 or x.shape[1:] != (128, 128, 3):
            raise ValueError("expected input of shape [N,128,128,3], got %r" % (x.shape,))
        n = x.shape[0]
        xyz = np.empty((n, 128, 128, 3), np.float32)
        prob = np.empty((n, 128, 128, 1), np.float32)
        _lib.check(_lib.lib().p2p_predict(self.ctx.handle, self._h, x.ctypes.data, n, xyz.ctypes.data,
                                          prob.ctypes.data, _lib.MEM_HOST), "p2p_predict")
        return [xyz, prob]

    @property
    def active_precision(self) -> str:
        """'f32' or 'f16x3': what the next pass computes in (an 'auto' generator reports 'f16x3' until a range event)."""
        return "f32" if _lib.lib().p2p_model_precision(self._h) == 0 else "f16x3"

    def forward_device(self, x_ptr: int, n: int, xyzp_ptr: int):
        """Asynchronous forward on device pointers (ints), interleaved [n,128,128,4] output."""
        _lib.check(_lib.lib().p2p_forward_async(self.ctx.handle, self._h, x_ptr, n, xyzp_ptr), "p2p_forward_async")

    def close(self):
        if self._h:
            _lib.lib().p2p_model_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------------------------------------
# batched pose estimation (C ABI: p2p_est_pose_batch / p2p_pnp_ransac_batch)
# --------------------------------------------------------------------------------------------
class ObjectSpec:
    """What one reference ``pix2pose`` instance holds per object (recognition.py:10-26)."""

    def __init__(self, generator: Generator, obj_param, th_outlier=(0.1, 0.2, 0.3), th_inlier=0.1, box_size=1.5):
        th_outlier = list(th_outlier)
        if not 1 <= len(th_outlier) <= _lib.MAX_TH:
            raise ValueError("th_outlier must hold 1..%d thresholds" % _lib.MAX_TH)
        self.generator = generator
        self.obj_param = np.asarray(obj_param, np.float64).reshape(6)
        self.th_outlier = [float(t) for t in th_outlier]
        self.th_inlier = float(th_inlier)
        self.box_size = float(box_size)

    def as_struct(self) -> "_lib.Object":
        o = _lib.Object()
        o.model = self.generator.handle
        for k in range(3):
            o.obj_scale[k] = self.obj_param[k]
            o.obj_ct[k] = self.obj_param[3 + k]
        o.n_outlier_th = len(self.th_outlier)
        for k, t in enumerate(self.th_outlier):
            o.outlier_th[k] = t
        o.inlier_th = self.th_inlier
        o.box_size = self.box_size
        return o


def _image_struct(img):
    """numpy HxWx3 uint8/float32 array, or (device_ptr, H, W, 'u8'|'f32') for a frame already in HBM."""
    s = _lib.Image()
    if isinstance(img, tuple):
        ptr, h, w, dt = img
        s.data, s.height, s.width = ptr, h, w
        s.dtype = 1 if dt == "f32" else 0
        s.mem = _lib.MEM_DEVICE
        return s, None
    a = np.asarray(img)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("image must be HxWx3, got %r" % (a.shape,))
    if a.dtype == np.uint8:
        a = np.ascontiguousarray(a)
        s.dtype = 0
    else:
        a = np.ascontiguousarray(a, dtype=np.float32)
        s.dtype = 1
    s.data, s.height, s.width, s.mem = a.ctypes.data, a.shape[0], a.shape[1], _lib.MEM_HOST
    return s, a


# skimage.transform.resize GENERATION (p2p_est_pose_opts.resize_anti_aliasing; include/p2p_mi355.h has the full account).  The reference calls
# resize six times per detection and does not pin scikit-image, so the caller names the library its reference environment resolves to.
RESIZE_GENERATIONS = {"0.14": 0, "0.15": 2, "0.16": 2, "0.17": 1, "0.18": 1}
_warned_unpinned = False


def resize_generation(spec) -> int:
    """None / False / 0 / "0.14" -> 0 (scikit-image <= 0.14: no anti-aliasing, every image warped in double; pinned to the real 0.18.3 float64 warp);
    True / 1 / "0.17" / "0.18" -> 1 (pinned bit for bit to the real 0.18.3); 2 / "0.15" / "0.16" -> 2 (anti-aliasing on for every input
    including the bool keep mask; its Gaussian filter pinned to the real scipy, its warp restated)."""
    if spec is None or spec is False:
        return 0
    if spec is True:
        return 1
    if isinstance(spec, str):
        if spec not in RESIZE_GENERATIONS:
            raise ValueError("skimage must be one of %s (>= 0.19 rejects the reference's bool mask resize), got %r" % (sorted(RESIZE_GENERATIONS), spec))
        return RESIZE_GENERATIONS[spec]
    g = int(spec)
    if g not in (0, 1, 2):
        raise ValueError("resize generation must be 0, 1 or 2, got %r" % (spec,))
    return g


def warn_unpinned_generation(who: str):
    """The reference does not pin scikit-image and its six resize calls differ between the library's generations: a caller that names none gets
    the <= 0.14 semantics (pinned to the real library's float64 warp like the others) -- say so, once."""
    global _warned_unpinned
    if not _warned_unpinned:
        _warned_unpinned = True
        import warnings
        warnings.warn("%s: no scikit-image generation was named -- using the <= 0.14 resize semantics (no anti-aliasing filter).  The reference "
                      "does not pin scikit-image and the generations give different masks: name the version the reference environment "
                      "resolves to (skimage='0.14', '0.15' / '0.16' -- what the reference's python-3.5 image installs -- or '0.17' / '0.18') "
                      "to silence this" % who, stacklevel=3)


def _marshal(objects, images, detections, inject1, inject2, inject_slots, want_masks, det_masks, ransac_iterations,
             reprojection_error, confidence, anti_aliasing=False):
    """Build the C arrays of one batch call.  -> (objs, imgs, dets, opts, extras, keep-alive list)"""
    n = len(detections)
    if ransac_iterations > _lib.MAX_RANSAC_ITERATIONS:
        raise ValueError("ransac_iterations %d exceeds the library's limit of %d" % (ransac_iterations, _lib.MAX_RANSAC_ITERATIONS))
    objs = (_lib.Object * max(len(objects), 1))(*[o.as_struct() for o in objects])
    keep = [objects, images]
    imgs = (_lib.Image * max(len(images), 1))()
    for i, im in enumerate(images):
        imgs[i], a = _image_struct(im)
        keep.append(a)
    dets = (_lib.Detection * max(n, 1))()
    if n:      # one vectorised fill instead of 15 ctypes assignments per detection
        dv = np.frombuffer(dets, dtype=_lib.DETECTION_DTYPE, count=n)
        dv["image"] = [d[0] for d in detections]
        dv["object"] = [d[1] for d in detections]
        dv["bbox"] = np.array([[int(b) for b in d[2]] for d in detections], np.int32).reshape(n, 4)     # int() truncation like the reference's roi.astype(np.int)
        dv["camK"] = np.array([np.asarray(d[3], np.float64).reshape(9) for d in detections], np.float64)
    opts = _lib.EstPoseOpts()
    opts.ransac_iterations, opts.reprojection_error, opts.confidence = ransac_iterations, reprojection_error, confidence
    opts.inject1, opts.inject2, opts.inject_slots = inject1, inject2, inject_slots
    opts.resize_anti_aliasing = resize_generation(anti_aliasing)
    extras = {}
    if want_masks and n:
        def hw(i):
            im = images[detections[i][0]]
            return (im[1], im[2]) if isinstance(im, tuple) else np.asarray(im).shape[:2]
        mstride = max(hw(i)[0] * hw(i)[1] for i in range(n))

        def side(i):      # stage-1 square of the detection (get_boxes, recognition.py:28-43): the stage-2 crop never exceeds it
            _, oi, b, _ = detections[i]
            bs = objects[oi].box_size if 0 <= oi < len(objects) else 1.5
            return 2 * int(min(9999, max((b[3] - b[1]) * bs, (b[2] - b[0]) * bs)) / 2)
        pstride = 3 * min(mstride, max(max(side(i), 1) ** 2 for i in range(n)))
        extras["valid_mask"] = np.zeros((n, mstride), np.uint8)
        extras["img_pred"] = np.zeros((n, pstride), np.uint8)
        opts.valid_mask, opts.mask_stride = extras["valid_mask"].ctypes.data, mstride
        opts.mask_prezeroed = 1          # np.zeros above: fresh zero pages, the library writes the crop rows only
        opts.img_pred, opts.pred_stride = extras["img_pred"].ctypes.data, pstride
    if det_masks is not None and n:
        # score_type 2: IoU of each detector mask with valid_mask_full, computed on the device
        dms = max(int(np.asarray(m).size) for m in det_masks)
        dm = np.zeros((n, dms), np.uint8)
        for i, m in enumerate(det_masks):
            im = images[detections[i][0]]
            hw = (im[1], im[2]) if isinstance(im, tuple) else tuple(np.asarray(im).shape[:2])
            if tuple(np.asarray(m).shape[:2]) != tuple(hw):
                # the device reads the mask with the frame's row stride; the reference resizes such masks to the frame first
                # (tools/5_evaluation_bop_basic.py:309-310) -- that resize is left to the caller; a mismatch is an error here, not a silent misread
                raise ValueError("detector mask %d has shape %r, its frame %r" % (i, tuple(np.asarray(m).shape[:2]), tuple(hw)))
            mm = np.ascontiguousarray(np.asarray(m) != 0, dtype=np.uint8).reshape(-1)
            dm[i, :mm.size] = mm
        extras["mask_stats"] = np.zeros((n, 3), np.int64)
        extras["_dm"] = dm
        opts.det_mask, opts.det_mask_stride = dm.ctypes.data, dms
        opts.mask_stats = extras["mask_stats"].ctypes.data
    return objs, imgs, dets, opts, extras, keep


def est_pose_batch(ctx: Context, objects, images, detections, *, inject1=None, inject2=None, inject_slots=0,
                   want_masks=False, debug=False, ransac_iterations=0, reprojection_error=0.0, confidence=0.0,
                   det_masks=None, anti_aliasing=False):
    """detections: list of (image_idx, object_idx, bbox[v1,u1,v2,u2], camK 3x3).
    anti_aliasing: scikit-image 0.17-0.18 resize semantics (Gaussian pre-filter when down-scaling); default = <= 0.14.
    Returns (poses: list[_lib.Pose], extras: dict)."""
    n = len(detections)
    objs, imgs, dets, opts, extras, keep = _marshal(objects, images, detections, inject1, inject2, inject_slots, want_masks,
                                                    det_masks, ransac_iterations, reprojection_error, confidence, anti_aliasing)
    poses = (_lib.Pose * max(n, 1))()
    K = max([len(o.th_outlier) for o in objects], default=0)
    if debug and n:
        extras["x1"] = np.zeros((n, 128, 128, 3), np.float32)
        extras["x2"] = np.zeros((n, K, 128, 128, 3), np.float32)
        extras["boxes2"] = np.zeros((n, 12), np.int32)
        extras["cand"] = np.zeros((n, K, 6), np.int32)
        opts.dbg_x1, opts.dbg_x2 = extras["x1"].ctypes.data, extras["x2"].ctypes.data
        opts.dbg_boxes2, opts.dbg_cand = extras["boxes2"].ctypes.data, extras["cand"].ctypes.data
        extras["y1"] = np.zeros((n, 128, 128, 4), np.float32)
        extras["y2"] = np.zeros((n, K, 128, 128, 4), np.float32)
        opts.dbg_y1, opts.dbg_y2 = extras["y1"].ctypes.data, extras["y2"].ctypes.data
    _lib.check(_lib.lib().p2p_est_pose_batch(ctx.handle, objs, len(objects), imgs, len(images), dets, n, poses,
                                             C.byref(opts)), "p2p_est_pose_batch")
    return [poses[i] for i in range(n)], extras


class Comm:
    """RCCL communicator of the C ABI (p2p_comm_*): one per rank, on the rank's context.  ``Comm.unique_id()`` on rank 0, the 128 bytes
    handed to every rank by the host program, ``Comm(ctx, rank, world, id)`` on all of them (collective)."""

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
        _lib.check(_lib.lib().p2p_comm_unique_id(buf), "p2p_comm_unique_id")
        return buf.raw

    def __init__(self, ctx: Context, rank: int, world: int, uid: bytes):
        if len(uid) != _lib.COMM_ID_BYTES:
            raise ValueError("the communicator id has %d bytes" % _lib.COMM_ID_BYTES)
        self.ctx, self.rank, self.world = ctx, rank, world
        self._h = C.c_void_p()
        _lib.check(_lib.lib().p2p_comm_create(ctx.handle, rank, world, uid, C.byref(self._h)), "p2p_comm_create")

    @property
    def handle(self):
        return self._h

    @staticmethod
    def library() -> str:
        return (_lib.lib().p2p_comm_library() or b"").decode()

    def close(self):
        if self._h:
            _lib.lib().p2p_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PendingBatch:
    """Handle of a batch enqueued with est_pose_submit (keeps the argument and output buffers alive)."""

    def __init__(self, ctx, ticket, n, keep, extras):
        self.ctx, self.ticket, self.n, self._keep, self.extras = ctx, ticket, n, keep, extras

    def collect(self):
        """Wait for the batch; -> list of p2p_pose records in the caller's detection order.  The optional outputs
        requested at submit time (valid_mask / img_pred / mask_stats) are in ``self.extras`` afterwards."""
        poses = (_lib.Pose * max(self.n, 1))()
        _lib.check(_lib.lib().p2p_est_pose_collect(self.ctx.handle, self.ticket, poses), "p2p_est_pose_collect")
        self._keep = None
        self.pose_array = poses          # the ctypes array itself (parallel.poses_to_records takes it without a Python loop)
        return [poses[i] for i in range(self.n)]

    def collect_gathered(self, comm: "Comm", n_max: int):
        """collect() + the RCCL all-gather of every rank's records (p2p_est_pose_collect_gathered: device to device on the batch's tail
        stream, one D2H afterwards).  Collective.  -> (this rank's poses, ctypes array of world * n_max records in rank order, each
        rank's block in its caller's detection order, padded with status = POSE_ABSENT)."""
        poses = (_lib.Pose * max(self.n, 1))()
        allp = (_lib.Pose * (comm.world * n_max))()
        _lib.check(_lib.lib().p2p_est_pose_collect_gathered(self.ctx.handle, comm.handle, self.ticket, poses, n_max, allp),
                   "p2p_est_pose_collect_gathered")
        self._keep = None
        self.pose_array = poses
        return [poses[i] for i in range(self.n)], allp


def collect_gathered_empty(ctx: Context, comm: "Comm", n_max: int):
    """This rank has NO batch this step (an empty shard: its images ran out, or none of its detections survived the candidate limits)
    but its peers do: join their p2p_est_pose_collect_gathered with ticket = P2P_TICKET_NONE, contributing n_max padding records.
    Collective.  -> ctypes array of world * n_max records as from PendingBatch.collect_gathered."""
    allp = (_lib.Pose * (comm.world * n_max))()
    _lib.check(_lib.lib().p2p_est_pose_collect_gathered(ctx.handle, comm.handle, _lib.TICKET_NONE, None, n_max, allp),
               "p2p_est_pose_collect_gathered(empty shard)")
    return allp


def est_pose_submit(ctx: Context, objects, images, detections, *, inject1=None, inject2=None, inject_slots=0,
                    ransac_iterations=0, reprojection_error=0.0, confidence=0.0, want_masks=False, det_masks=None,
                    anti_aliasing=False, merge_passes=False) -> PendingBatch:
    """Asynchronous est_pose_batch for detection streams: enqueue and return; at most two batches in
    flight per context.  The PnP-RANSAC tail of this batch overlaps the generator passes of the next.
    ``want_masks`` / ``det_masks`` as in est_pose_batch: the arrays in ``PendingBatch.extras`` are filled by collect()."""
    n = len(detections)
    objs, imgs, dets, opts, extras, keep = _marshal(objects, images, detections, inject1, inject2, inject_slots, want_masks,
                                                    det_masks, ransac_iterations, reprojection_error, confidence, anti_aliasing)
    opts.merge_stream_passes = 1 if merge_passes else 0       # the next submit may run this batch's stage-2 pass merged with its stage-1 pass
    ticket = C.c_int(-1)
    _lib.check(_lib.lib().p2p_est_pose_submit(ctx.handle, objs, len(objects), imgs, len(images), dets, n, C.byref(opts),
                                              C.byref(ticket)), "p2p_est_pose_submit")
    keep += [objs, imgs, dets, opts]
    return PendingBatch(ctx, ticket.value, n, keep, extras)


def pnp_ransac_batch(ctx: Context, Ks, objs, imgs, iterations=100, reproj_err=5.0, confidence=0.99, want_mask=False):
    """Batch of independent cv2.solvePnPRansac(EPNP) problems on the GPU.
    -> ok [P] bool, R [P,3,3], t [P,3], info [P,3] (n_inliers, iterations, best_iter), masks list|None"""
    n_prob = len(objs)
    offsets = np.zeros(n_prob + 1, np.int32)
    offsets[1:] = np.cumsum([len(o) for o in objs])
    obj = np.ascontiguousarray(np.concatenate(objs) if n_prob else np.zeros((0, 3)), np.float64).reshape(-1, 3)
    img = np.ascontiguousarray(np.concatenate(imgs) if n_prob else np.zeros((0, 2)), np.float64).reshape(-1, 2)
    K = np.ascontiguousarray(Ks, np.float64).reshape(n_prob, 9)
    R = np.zeros((n_prob, 9)); t = np.zeros((n_prob, 3))
    info = np.zeros((n_prob, 3), np.int32); ok = np.zeros(n_prob, np.int32)
    mask = np.zeros(max(int(offsets[-1]), 1), np.uint8) if want_mask else None
    dp = C.POINTER(C.c_double)
    ip = C.POINTER(C.c_int)
    _lib.check(_lib.lib().p2p_pnp_ransac_batch(ctx.handle, K.ctypes.data_as(dp), obj.ctypes.data_as(dp),
                                               img.ctypes.data_as(dp), offsets.ctypes.data_as(ip), n_prob, iterations,
                                               reproj_err, confidence, R.ctypes.data_as(dp), t.ctypes.data_as(dp),
                                               info.ctypes.data_as(ip), ok.ctypes.data_as(ip),
                                               mask.ctypes.data if want_mask else None), "p2p_pnp_ransac_batch")
    masks = [mask[offsets[i]:offsets[i + 1]] for i in range(n_prob)] if want_mask else None
    return ok.astype(bool), R.reshape(-1, 3, 3), t, info, masks


class Mesh:
    """An object's triangle mesh in HBM (p2p_mesh_create): verts [N,3] in mm (cast to float32), tris [M,3] vertex indices.
    ``Mesh.from_ply(ctx, path)`` reads a BOP ``obj_<id:06d>.ply`` through pix2pose_amd.mesh.read_ply."""

    def __init__(self, ctx: Context, verts, tris):
        self.ctx = ctx
        v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
        self.n_verts, self.n_tris = len(v), len(f)
        self._h = C.c_void_p()
        _lib.check(_lib.lib().p2p_mesh_create(ctx.handle, v.ctypes.data, len(v), f.ctypes.data, len(f), C.byref(self._h)),
                   "p2p_mesh_create")

    @classmethod
    def from_ply(cls, ctx: Context, path: str) -> "Mesh":
        from .mesh import read_ply
        return cls(ctx, *read_ply(path))

    @classmethod
    def from_xyz_ply(cls, ctx: Context, path: str) -> "Mesh":
        """A models_xyz PLY (pix2pose_amd.xyz_model): the mesh with its vertex colours set."""
        from .xyz_model import read_xyz_model
        verts, tris, colors = read_xyz_model(path)
        m = cls(ctx, verts, tris)
        m.set_colors(colors)
        return m

    def set_colors(self, colors) -> None:
        """Per-vertex colours uint8 [N,3] (p2p_mesh_set_colors), what render_xyz_batch interpolates; N must be the vertex count."""
        c = np.asarray(colors)
        if c.dtype != np.uint8:
            raise ValueError("vertex colours must be uint8, got %s" % c.dtype)
        c = np.ascontiguousarray(c).reshape(-1, 3)
        _lib.check(_lib.lib().p2p_mesh_set_colors(self._h, c.ctypes.data, len(c)), "p2p_mesh_set_colors")

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            _lib.lib().p2p_mesh_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _depth_jobs(jobs, keep):
    """jobs: sequence of dicts {mesh, camK [3,3], R [3,3], t [3] in mm (p2p_pose units), image, union_mask} -> p2p_refine_job[]."""
    arr = (_lib.RefineJob * max(1, len(jobs)))()
    for k, j in enumerate(jobs):
        arr[k].mesh_idx = int(j["mesh"])
        arr[k].img_idx = int(j.get("image", 0))
        arr[k].camK[:] = [float(x) for x in np.asarray(j["camK"], np.float64).ravel()]
        arr[k].R[:] = [float(x) for x in np.asarray(j["R"], np.float64).ravel()]
        arr[k].t[:] = [float(x) for x in np.asarray(j["t"], np.float64).ravel()]
        m = j.get("union_mask")
        if m is not None:
            m = np.ascontiguousarray(np.asarray(m) != 0, dtype=np.uint8)
            keep.append(m)
            arr[k].union_mask = m.ctypes.data
    return arr


def render_depth_batch(ctx: Context, meshes, jobs, height: int, width: int):
    """Depth-only z-buffer (p2p_render_depth_batch; replaces render_obj(), icp3d.py:40-50): float32 [n_jobs, H, W] in metres, 0 where
    nothing is drawn.  jobs as in _depth_jobs (image / union_mask unused)."""
    keep = []
    arr = _depth_jobs(jobs, keep)
    mh = (C.c_void_p * max(1, len(meshes)))(*[m.handle.value for m in meshes])
    out = np.zeros((len(jobs), height, width), np.float32)
    _lib.check(_lib.lib().p2p_render_depth_batch(ctx.handle, mh, len(meshes), arr, len(jobs), height, width, out.ctypes.data),
               "p2p_render_depth_batch")
    return out


def render_xyz_batch(ctx: Context, meshes, jobs, height: int, width: int):
    """Colour z-buffer of XYZ-coloured meshes (p2p_render_xyz_batch; replaces get_rendering() of the reference's
    2_2_render_pix2pose_training.py): -> (color float32 [n, H, W, 3] in [0, 1], channels (x, y, z), 0 where nothing is drawn;
    depth float32 [n, H, W], bit-identical to render_depth_batch; bbox int32 [n, 4] = [min v, min u, max v, max u] of depth > 0,
    max inclusive, -1s for an empty render).  jobs as in render_depth_batch; every mesh needs set_colors first."""
    keep = []
    arr = _depth_jobs(jobs, keep)
    mh = (C.c_void_p * max(1, len(meshes)))(*[m.handle.value for m in meshes])
    color = np.zeros((len(jobs), height, width, 3), np.float32)
    depth = np.zeros((len(jobs), height, width), np.float32)
    bbox = np.full((len(jobs), 4), -1, np.int32)
    _lib.check(_lib.lib().p2p_render_xyz_batch(ctx.handle, mh, len(meshes), arr, len(jobs), height, width, color.ctypes.data,
                                               depth.ctypes.data, bbox.ctypes.data), "p2p_render_xyz_batch")
    return color, depth, bbox


def xyz_patch_batch(ctx: Context, rgbs, color, depth, bbox, generation: int = 0):
    """Training patches of colour renders (p2p_xyz_patch_batch; 2_2_render_pix2pose_training.py:168-184): rgbs[k] uint8 [H, W, 3],
    and color / depth / bbox as render_xyz_batch returned them for the same jobs.  -> a list with, per job, the uint8 [h, w, 6]
    patch ([rgb | xyz], at most 128 on its longer side) or None for a job that is skipped (empty render, or a box with a zero
    side).  generation: the scikit-image resize generation of boxes above 128 px (runtime.resize_generation)."""
    n = len(rgbs)
    color = np.ascontiguousarray(color, dtype=np.float32)
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    bbox = np.ascontiguousarray(bbox, dtype=np.int32).reshape(-1, 4)
    if n == 0:
        return []
    H, W = depth.shape[1:]
    if color.shape != (n, H, W, 3) or depth.shape != (n, H, W) or len(bbox) != n:
        raise ValueError("color / depth / bbox do not describe %d renders of one size" % n)
    rgbs = [np.ascontiguousarray(r, dtype=np.uint8) for r in rgbs]
    if any(r.shape != (H, W, 3) for r in rgbs):
        raise ValueError("every frame must be uint8 [%d, %d, 3]" % (H, W))
    rp = (C.c_void_p * n)(*[r.ctypes.data for r in rgbs])
    out = np.zeros((n, 128, 128, 6), np.uint8)
    shapes = np.zeros((n, 2), np.int32)
    _lib.check(_lib.lib().p2p_xyz_patch_batch(ctx.handle, rp, color.ctypes.data, depth.ctypes.data, bbox.ctypes.data, n, H, W,
                                              int(generation), out.ctypes.data, shapes.ctypes.data), "p2p_xyz_patch_batch")
    return [out[k, :shapes[k, 0], :shapes[k, 1]].copy() if shapes[k, 0] > 0 else None for k in range(n)]


def _rot_mm(a, b):
    """a @ b in plain double products summed in index order, no fused multiply-add: what numpy's matmul gave under the library for
    these 3-column operands, written out so that the bits do not depend on the BLAS underneath."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.zeros((a.shape[0], b.shape[1]))
    for i in range(a.shape[0]):
        for j in range(b.shape[1]):
            s = float(a[i, 0]) * float(b[0, j])
            for k in range(1, a.shape[1]):
                s = s + float(a[i, k]) * float(b[k, j])
            out[i, j] = s
    return out


def _rot_inv3(m):
    """np.linalg.inv of a 3 x 3 matrix as LAPACK's dgesv computes it (held bit for bit to numpy 1.26 / OpenBLAS on the matrices of
    rotate): LU with partial pivoting, the column below a pivot scaled by the pivot's reciprocal, plain multiply-subtract updates,
    then per column of the identity the forward substitution and a back substitution that multiplies by the diagonal's reciprocal."""
    n = 3
    A = [[float(m[i][j]) for j in range(n)] for i in range(n)]
    B = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    for k in range(n):
        p = max(range(k, n), key=lambda i: (abs(A[i][k]), -i))
        if p != k:
            A[k], A[p] = A[p], A[k]
            B[k], B[p] = B[p], B[k]
        r = 1.0 / A[k][k]
        for i in range(k + 1, n):
            A[i][k] = A[i][k] * r
        for i in range(k + 1, n):
            for j in range(k + 1, n):
                A[i][j] = A[i][j] - A[i][k] * A[k][j]
    for c in range(n):
        for k in range(n):
            for i in range(k + 1, n):
                B[i][c] = B[i][c] - A[i][k] * B[k][c]
        for k in range(n - 1, -1, -1):
            B[k][c] = B[k][c] * (1.0 / A[k][k])
            for i in range(k):
                B[i][c] = B[i][c] - A[i][k] * B[k][c]
    return np.array(B)


def skimage_rotate_matrix(rows: int, cols: int, angle: float):
    """What skimage.transform.rotate(image [rows, cols], angle, resize=True) of scikit-image 0.17 / 0.18 hands to its warp, with the
    library's operations in the library's order (its matmul and linalg.inv written out in plain double arithmetic, _rot_mm and
    _rot_inv3, so that the bits do not depend on the BLAS / LAPACK build under numpy): -> (float64 [3, 3] map from (x, y, 1) of the rotated image to (column, row,
    1) of the input, (out_rows, out_cols)).  tform3 + tform2 + tform1 is t1 @ (t2 @ t3) in that association (a + b multiplies
    b.params @ a.params), the shape comes from the inverse image of the four corners, and the translation to the corner minimum is
    multiplied on the right."""
    def translation(tx, ty):
        m = np.array([[1.0, -0.0, 0], [0.0, 1.0, 0], [0, 0, 1]])
        m[0:2, 2] = (tx, ty)
        return m
    a = np.deg2rad(angle)
    center = np.array((cols, rows)) / 2. - 0.5
    t2 = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    m = _rot_mm(translation(*center), _rot_mm(t2, translation(*(-center))))
    corners = np.array([[0, 0], [0, rows - 1], [cols - 1, rows - 1], [cols - 1, 0]])
    x, y = np.transpose(corners)
    dst = _rot_mm(np.vstack((x, y, np.ones_like(x))).T, _rot_inv3(m).T)
    dst[dst[:, 2] == 0, 2] = np.finfo(float).eps
    dst[:, :2] /= dst[:, 2:3]
    minc, minr, maxc, maxr = dst[:, 0].min(), dst[:, 1].min(), dst[:, 0].max(), dst[:, 1].max()
    shape = np.around((maxr - minr + 1, maxc - minc + 1)).astype(int)
    m = _rot_mm(m, translation(minc, minr))
    m[2] = (0, 0, 1)
    return m, (int(shape[0]), int(shape[1]))


def rotate_input_tables():
    """The float32 value of the two images the reference's augment_inplane_gen rotates, per 8-bit level q: (rgb, xyz), float32 [256]
    each.  rgb: (img / 255).astype(float32) of the uint8 frame.  xyz: the render is read back as float32(q) / 255, multiplied by 255 in
    float32 (get_rendering), and (img_r / 255) divides that float32 array again."""
    q = np.arange(256)
    rgb = (q.astype(np.uint8) / 255).astype(np.float32)
    qf = q.astype(np.float32)
    xyz = ((qf / np.float32(255)) * np.float32(255)) / np.float32(255)
    return np.ascontiguousarray(rgb), np.ascontiguousarray(xyz, dtype=np.float32)


def xyz_rotate_patch_batch(ctx: Context, rgbs, color, depth, angles, generation: int = 1):
    """The in-plane rotation copies of the training patches (p2p_xyz_rotate_patch_batch; 2_2_render_pix2pose_training.py:64-96):
    rgbs / color / depth as for xyz_patch_batch, angles[k] the rotations of job k in degrees (lists of different lengths are fine,
    an empty one too).  -> per job a list with, per angle, the uint8 [h, w, 6] patch or None (empty render, zero-sided box).
    generation must be 1 (scikit-image 0.17 / 0.18).  Frame and render travel to the device once per job."""
    n = len(rgbs)
    color = np.ascontiguousarray(color, dtype=np.float32)
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    if n == 0:
        return []
    if depth.ndim != 3:
        raise ValueError("depth must be float32 [n, H, W]")
    H, W = depth.shape[1:]
    if color.shape != (n, H, W, 3) or depth.shape != (n, H, W) or len(angles) != n:
        raise ValueError("color / depth / angles do not describe %d renders of one size" % n)
    rgbs = [np.ascontiguousarray(r, dtype=np.uint8) for r in rgbs]
    if any(r.shape != (H, W, 3) for r in rgbs):
        raise ValueError("every frame must be uint8 [%d, %d, 3]" % (H, W))
    counts = np.array([len(a) for a in angles], np.int32)
    total = int(counts.sum())
    mats = np.zeros((max(1, total), 6), np.float64)
    rshapes = np.zeros((max(1, total), 2), np.int32)
    cache = {}
    i = 0
    for a_list in angles:
        for a in a_list:
            a = float(a)
            if a not in cache:
                if np.isfinite(a):
                    m, s = skimage_rotate_matrix(H, W, a)
                    cache[a] = (m[:2].ravel(), s)
                else:
                    cache[a] = (np.full(6, np.nan), (0, 0))        # the library call names the bad angle list
            mats[i], rshapes[i] = cache[a]
            i += 1
    rgb_tab, xyz_tab = rotate_input_tables()
    rp = (C.c_void_p * n)(*[r.ctypes.data for r in rgbs])
    out = np.zeros((max(1, total), 128, 128, 6), np.uint8)
    shapes = np.zeros((max(1, total), 2), np.int32)
    _lib.check(_lib.lib().p2p_xyz_rotate_patch_batch(ctx.handle, rp, color.ctypes.data, depth.ctypes.data, n, H, W, counts.ctypes.data,
                                                     mats.ctypes.data, rshapes.ctypes.data, rgb_tab.ctypes.data, xyz_tab.ctypes.data,
                                                     int(generation), out.ctypes.data, shapes.ctypes.data), "p2p_xyz_rotate_patch_batch")
    res, i = [], 0
    for a_list in angles:
        res.append([out[i + j, :shapes[i + j, 0], :shapes[i + j, 1]].copy() if shapes[i + j, 0] > 0 else None for j in range(len(a_list))])
        i += len(a_list)
    return res


def train_frame_shape(patch_shape, back_shape):
    """(rows, columns) of the background after data_io.py:78-85: an axis shorter than twice the patch is stretched to twice the patch."""
    ph, pw = int(patch_shape[0]), int(patch_shape[1])
    H, W = int(back_shape[0]), int(back_shape[1])
    if H < 2 * ph or W < 2 * pw:
        return max(2 * ph if H < 2 * ph else 0, H), max(2 * pw if W < 2 * pw else 0, W)
    return H, W


def train_rotate_matrix(side: int, angle: float):
    """Rows 0 and 1 (6 doubles) of what skimage.transform.rotate(image [side, side], angle) -- no resize -- hands to its warp:
    t1 @ (t2 @ t3) in that association, as skimage_rotate_matrix forms it before its corner step."""
    def translation(tx, ty):
        m = np.array([[1.0, -0.0, 0], [0.0, 1.0, 0], [0, 0, 1]])
        m[0:2, 2] = (tx, ty)
        return m
    a = np.deg2rad(angle)
    center = np.array((side, side)) / 2. - 0.5
    t2 = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    m = _rot_mm(translation(*center), _rot_mm(t2, translation(*(-center))))
    return m[:2].ravel()


def train_draws(rand, patch_shape, back_shape, batch_count: int):
    """One sample's draws of data_io.py: get_patch_pair, taken from `rand` (the `random` module or a random.Random: .random() and
    .gauss()) in the reference's order and turned into integers by the reference's int(...) expressions in Python floats.
    back_shape: the background's (H, W[, C]), or a callable that receives the first draw (the background index is
    int(draw * (n_background - 1)), :71) and returns that shape.  -> dict: the fields of p2p_train_draw (rect holds the three
    rectangles with Python's slice rule applied to the frame), 'frame' (rows, columns after the enlargement rule), 'angle', and
    'draws', the raw values in the order they were consumed."""
    raw = []

    def rnd():
        raw.append(rand.random())
        return raw[-1]
    ph, pw = int(patch_shape[0]), int(patch_shape[1])
    first = rnd()
    shape = back_shape(first) if callable(back_shape) else back_shape
    Hb, Wb = train_frame_shape((ph, pw), shape)
    v_ref = int(rnd() * (Hb - ph - 20) + 10)
    u_ref = int(rnd() * (Wb - pw - 20) + 10)
    box = (v_ref, u_ref, v_ref + ph, u_ref + pw)
    ct_v = int((box[0] + box[2]) / 2 + (rnd() * 10 - 5))
    ct_u = int((box[1] + box[3]) / 2 + (rnd() * 10 - 5))
    width = (box[3] - box[1]) * (1 + (rnd() * 0.6 - 0.3))
    height = (box[2] - box[0]) * (1 + (rnd() * 0.6 - 0.3))
    h = w = max(width * 1.5, height * 1.5)
    v1, v2, u1, u2 = ct_v - int(h / 2), ct_v + int(h / 2), ct_u - int(w / 2), ct_u + int(w / 2)
    side = v2 - v1
    shift_v = shift_u = 0
    if v1 < 0:
        shift_v, v1 = abs(v1), 0
    v2 = min(v2, Hb)
    if u1 < 0:
        shift_u, u1 = abs(u1), 0
    u2 = min(u2, Wb)

    def rectangle(low):
        h_aug = int((rnd() * 0.5 + low) * h)
        w_aug = int((rnd() * 0.5 + low) * w)
        ratio = 0.5
        d_v = int(int((box[0] + box[2]) / 2) + (rnd() * ratio * 2 - ratio) * height)
        d_u = int(int((box[1] + box[3]) / 2) + (rnd() * ratio * 2 - ratio) * width)
        if not (h_aug > 0 and w_aug > 0):
            return [0, 0, 0, 0]
        r0, r1, _ = slice(d_v, d_v + h_aug).indices(Hb)
        c0, c1, _ = slice(d_u, d_u + w_aug).indices(Wb)
        return [r0, r1, c0, c1] if r0 < r1 and c0 < c1 else [0, 0, 0, 0]
    rect = [rectangle(0.2), [0, 0, 0, 0], [0, 0, 0, 0]]
    sigma_edge = rnd() * 2
    sigma_blur = rnd() * 2
    even = batch_count % 2 == 0
    sigma_ran = 0.0
    if even:
        raw.append(rand.gauss(0.5, 0.3))
        sigma_ran = min(max(raw[-1], 0.1), 1.0)
        rect[1] = rectangle(0.0)
        rect[2] = rectangle(0.0)
    angle = rnd() * 30 - 15
    return {"v_ref": v_ref, "u_ref": u_ref, "v1": v1, "v2": v2, "u1": u1, "u2": u2, "side": side, "shift_v": shift_v, "shift_u": shift_u,
            "rect": rect, "even": int(even), "sigma_edge": sigma_edge, "sigma_blur": sigma_blur, "sigma_ran": sigma_ran, "angle": angle,
            "rot": train_rotate_matrix(side, angle) if side > 0 else np.full(6, np.nan), "frame": (Hb, Wb), "draws": raw}


TRAIN_COLOUR_IDS = ("add0", "add1", "add2", "contrast", "multiply", "blur", "noise", "contrast2")


def train_colours(rng, n: int, first_sample: int = 0):
    """n parameter records of the colour stage (seq_syn, data_io.py:42-51) from a numpy.random.Generator: a random order of the eight
    augmenters and imgaug's documented parameter ranges.  An explicitly unpinned restatement: imgaug's own random stream and float
    arithmetic are not reproduced.  -> list of dicts with the fields of p2p_train_colour."""
    out = []
    for k in range(n):
        rec = {"order": [int(v) for v in rng.permutation(8)], "add": [float(v) for v in rng.uniform(-15, 15, 3)],
               "contrast": float(rng.uniform(0.8, 1.3))}
        rec["mul"] = [float(v) for v in rng.uniform(0.8, 1.2, 3)] if rng.random() < 0.5 else [float(rng.uniform(0.8, 1.2))] * 3
        rec["blur_sigma"] = float(rng.uniform(0.0, 0.5))
        rec["noise_scale"] = 10.0 if rng.random() < 0.1 else 0.0
        if rng.random() < 0.5:
            rec["contrast2"] = [float(v) for v in rng.uniform(0.5, 2.2, 3)] if rng.random() < 0.3 else [float(rng.uniform(0.5, 2.2))] * 3
        else:
            rec["contrast2"] = [1.0, 1.0, 1.0]
        rec["sample"] = first_sample + k
        rec["seed"] = int(rng.integers(0, 2 ** 63))
        out.append(rec)
    return out


def train_patch_batch(ctx: Context, patches, backgrounds, draws, colours=None, imsize: int = 128, device: bool = False,
                      return_status: bool = False, generation: int = 1):
    """A batch of training samples in one library call (p2p_train_batch; data_io.py: get_patch_pair for scikit-image 0.17 / 0.18).
    patches: uint8 [h, w, 6 or 7] arrays as make_train_xyz writes them (h, w <= 128); backgrounds: uint8 [H, W, 3] or [H, W], one per
    sample (the same array may appear many times); draws: the records of train_draws; colours: None (the colour stage is skipped) or
    the records of train_colours -- that stage follows imgaug's documented meaning and is not pinned to it.
    -> (src [n, S, S, 3], tgt [n, S, S, 3], mask [n, S, S]) float32, S = imsize: numpy arrays, or with device=True torch tensors on
    the context's device that the kernels wrote directly.  A sample the library leaves out (a patch above 128, a background smaller
    than the patch plus 20 after the enlargement rule, a draw that is not finite or a window above 250) raises ValueError; with
    return_status=True its outputs are 0 and the int32 status array is returned as a fourth value."""
    n = len(patches)
    if len(backgrounds) != n or len(draws) != n or (colours is not None and len(colours) != n):
        raise ValueError("patches / backgrounds / draws / colours do not describe %d samples" % n)
    S = int(imsize)
    patches = [np.ascontiguousarray(p, dtype=np.uint8) for p in patches]
    backgrounds = [np.ascontiguousarray(b, dtype=np.uint8) for b in backgrounds]
    if any(p.ndim != 3 for p in patches) or any(b.ndim not in (2, 3) for b in backgrounds):
        raise ValueError("a patch must be [h, w, c] and a background [H, W, 3] or [H, W]")
    pshape = np.array([p.shape for p in patches], np.int32).reshape(n, 3)
    bshape = np.array([b.shape if b.ndim == 3 else b.shape + (1,) for b in backgrounds], np.int32).reshape(n, 3)
    dr = (_lib.TrainDraw * max(1, n))()
    for k, d in enumerate(draws):
        r = dr[k]
        for f in ("v_ref", "u_ref", "v1", "v2", "u1", "u2", "side", "shift_v", "shift_u", "even"):
            setattr(r, f, int(d[f]))
        for q in range(3):
            for e in range(4):
                r.rect[q][e] = int(d["rect"][q][e])
        r.sigma_edge, r.sigma_blur, r.sigma_ran = float(d["sigma_edge"]), float(d["sigma_blur"]), float(d["sigma_ran"])
        for q in range(6):
            r.rot[q] = float(d["rot"][q])
    co = None
    if colours is not None:
        co = (_lib.TrainColour * max(1, n))()
        for k, d in enumerate(colours):
            r = co[k]
            for q in range(8):
                r.order[q] = int(d["order"][q])
            for q in range(3):
                r.add[q], r.mul[q], r.contrast2[q] = float(d["add"][q]), float(d["mul"][q]), float(d["contrast2"][q])
            r.contrast, r.blur_sigma, r.noise_scale = float(d["contrast"]), float(d["blur_sigma"]), float(d["noise_scale"])
            r.sample, r.seed = int(d["sample"]) & 0xffffffff, int(d["seed"]) & 0xffffffffffffffff
    pp = (C.c_void_p * max(1, n))(*[p.ctypes.data for p in patches])
    bp = (C.c_void_p * max(1, n))(*[b.ctypes.data for b in backgrounds])
    status = np.zeros(max(1, n), np.int32)
    if device:
        import torch
        dev = torch.device("cuda", ctx.device)
        src = torch.empty((n, S, S, 3), dtype=torch.float32, device=dev)
        tgt = torch.empty((n, S, S, 3), dtype=torch.float32, device=dev)
        mask = torch.empty((n, S, S), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        ptrs = (src.data_ptr(), tgt.data_ptr(), mask.data_ptr())
    else:
        src, tgt, mask = np.zeros((n, S, S, 3), np.float32), np.zeros((n, S, S, 3), np.float32), np.zeros((n, S, S), np.float32)
        ptrs = (src.ctypes.data, tgt.ctypes.data, mask.ctypes.data)
    _lib.check(_lib.lib().p2p_train_batch(ctx.handle, n, pp, pshape.ctypes.data, bp, bshape.ctypes.data, dr, co, S, int(generation),
                                          ptrs[0], ptrs[1], ptrs[2], _lib.MEM_DEVICE if device else _lib.MEM_HOST, status.ctypes.data),
               "p2p_train_batch")
    status = status[:n]
    if return_status:
        return src, tgt, mask, status
    if n and status.any():
        msg = _lib.lib().p2p_last_error()
        raise ValueError("train_patch_batch: samples %s were left out (status %s): %s"
                         % (np.nonzero(status)[0].tolist(), status[status != 0].tolist(), msg.decode() if msg else "?"))
    return src, tgt, mask


def depth_score_batch(ctx: Context, meshes, depths, jobs, inlier_masks: bool = False):
    """Depth agreement at each job's pose (p2p_depth_score_batch; icp3d.py:470-490): renders the job and compares it with
    depths[job['image']] (float32 metres, depth_scale already applied) over job['union_mask'].  Returns a list of dicts
    {inlier_count, union, fcn, ratio} and, with inlier_masks=True, a bool array [n_jobs, H, W] as well."""
    depths = [np.ascontiguousarray(d, dtype=np.float32) for d in depths]
    if not depths:
        raise ValueError("depth_score_batch needs at least one depth image")
    H, W = depths[0].shape
    if any(d.shape != (H, W) for d in depths):
        raise ValueError("all depth images must have the same size")
    for j in jobs:
        if j.get("union_mask") is None or np.shape(j["union_mask"]) != (H, W):
            raise ValueError("every job needs a union_mask of the depth images' size %r" % ((H, W),))
    keep = []
    arr = _depth_jobs(jobs, keep)
    mh = (C.c_void_p * max(1, len(meshes)))(*[m.handle.value for m in meshes])
    dp = (C.c_void_p * len(depths))(*[d.ctypes.data for d in depths])
    res = (_lib.DepthScore * max(1, len(jobs)))()
    masks = np.zeros((len(jobs), H, W), np.uint8) if inlier_masks else None
    _lib.check(_lib.lib().p2p_depth_score_batch(ctx.handle, mh, len(meshes), dp, len(depths), arr, len(jobs), H, W, res,
                                                masks.ctypes.data if masks is not None else None), "p2p_depth_score_batch")
    out = [{"inlier_count": int(r.inlier_count), "union": int(r.union_count), "fcn": float(r.fcn), "ratio": float(r.ratio)}
           for r in res[:len(jobs)]]
    return (out, masks.astype(bool)) if inlier_masks else out


def depth_points_batch(ctx: Context, depths, camKs):
    """Scene points of whole frames (p2p_depth_points_batch; replaces getXYZ + get_normal(refine=True), icp3d.py:372-374): depths
    float32 [H, W] in metres, camKs [3, 3] each -> float32 [n, H, W, 6] = x y z nx ny nz."""
    depths = [np.ascontiguousarray(d, dtype=np.float32) for d in depths]
    if len(depths) != len(camKs):
        raise ValueError("one camera per depth image")
    if not depths:
        raise ValueError("depth_points_batch needs at least one depth image")
    H, W = depths[0].shape
    if any(d.shape != (H, W) for d in depths):
        raise ValueError("all depth images must have the same size")
    K = np.ascontiguousarray(np.asarray(camKs, np.float64).reshape(len(depths), 9))
    dp = (C.c_void_p * len(depths))(*[d.ctypes.data for d in depths])
    out = np.empty((len(depths), H, W, 6), np.float32)
    _lib.check(_lib.lib().p2p_depth_points_batch(ctx.handle, dp, len(depths), K.ctypes.data_as(C.POINTER(C.c_double)), H, W,
                                                 out.ctypes.data), "p2p_depth_points_batch")
    return out


def icp_inputs_batch(ctx: Context, meshes, depths, jobs):
    """The point sets of the ICP refinement (p2p_icp_inputs_batch; icp3d.py:464 and icp_refinement :58-85 up to registerModelToScene).
    depths: float32 [H, W] metres; jobs as in _depth_jobs, each with an 'image' and a 'union_mask' (depth_valid already ANDed in).
    Returns one dict per job: status (0, or _lib.ICP_SMALL_BBOX / ICP_FEW_POINTS, both the reference's -1), bbox, t_init, t_adjusted,
    centroid_src, centroid_tgt, and src / tgt float32 [k, 6] (x y z nx ny nz)."""
    depths = [np.ascontiguousarray(d, dtype=np.float32) for d in depths]
    if not depths:
        raise ValueError("icp_inputs_batch needs at least one depth image")
    H, W = depths[0].shape
    if any(d.shape != (H, W) for d in depths):
        raise ValueError("all depth images must have the same size")
    for j in jobs:
        if j.get("union_mask") is None or np.shape(j["union_mask"]) != (H, W):
            raise ValueError("every job needs a union_mask of the depth images' size %r" % ((H, W),))
    keep = []
    arr = _depth_jobs(jobs, keep)
    mh = (C.c_void_p * max(1, len(meshes)))(*[m.handle.value for m in meshes])
    dp = (C.c_void_p * len(depths))(*[d.ctypes.data for d in depths])
    res = (_lib.IcpInput * max(1, len(jobs)))()
    # init_mask is a subset of union_mask, so the union sizes bound both point sets; the retry covers a binding that guesses smaller
    n_tgt = sum(int(m.sum()) for m in keep)
    cap_src, cap_tgt = n_tgt, n_tgt
    while True:
        src = np.empty((max(cap_src, 1), 6), np.float32)
        tgt = np.empty((max(cap_tgt, 1), 6), np.float32)
        rc = _lib.lib().p2p_icp_inputs_batch(ctx.handle, mh, len(meshes), dp, len(depths), arr, len(jobs), H, W, res,
                                             src.ctypes.data, cap_src, tgt.ctypes.data, cap_tgt)
        if rc != _lib.ERR_CAPACITY:
            break
        recs = res[:len(jobs)]
        cap_src = max(cap_src, sum(int(r.n_src) for r in recs))
        cap_tgt = max(cap_tgt, sum(int(r.n_tgt) for r in recs))
    _lib.check(rc, "p2p_icp_inputs_batch")
    out = []
    for r in res[:len(jobs)]:
        out.append({"status": int(r.status), "bbox": list(r.bbox), "t_init": np.array(r.t_init[:]), "t_adjusted": np.array(r.t_adjusted[:]),
                    "centroid_src": np.array(r.centroid_src[:]), "centroid_tgt": np.array(r.centroid_tgt[:]),
                    "src": src[r.src_offset:r.src_offset + r.n_src].copy(), "tgt": tgt[r.tgt_offset:r.tgt_offset + r.n_tgt].copy()})
    return out


def _icp_params(max_iterations=100, tolerance=0.005, rejection_scale=2.5, num_levels=2):
    """cv2.ppf_match_3d_ICP(iterations, tolerence, rejectionScale, numLevels); the defaults are the reference's (icp3d.py:87)."""
    p = _lib.IcpParams()
    p.max_iterations, p.tolerance, p.rejection_scale, p.num_levels = int(max_iterations), tolerance, rejection_scale, int(num_levels)
    return p


def _icp_result(r):
    return {"status": int(r.status), "iterations": list(r.iterations), "pairs": list(r.pairs), "fval_min": list(r.fval_min),
            "scale": float(r.scale), "mean_avg": np.array(r.mean_avg[:]), "pose": np.array(r.pose[:]).reshape(4, 4)}


def icp_batch(ctx: Context, inputs, src=None, tgt=None, **params):
    """Point-to-plane ICP (p2p_icp_batch; the restatement of cv2.ppf_match_3d_ICP(...).registerModelToScene in DESIGN.md 8.2) of what
    icp_inputs_batch returns: inputs is its list of dicts (each with 'status', 'src', 'tgt'); src / tgt may instead give every job's
    point set [k, 6] explicitly.  params: max_iterations, tolerance, rejection_scale, num_levels (the reference's by default).
    Returns one dict per job: status, iterations / pairs / fval_min per level (index = level, 0 the finest), scale, mean_avg and pose
    (4 x 4, metres; identity when status != 0)."""
    n = len(inputs)
    src = [r["src"] for r in inputs] if src is None else src
    tgt = [r["tgt"] for r in inputs] if tgt is None else tgt
    if len(src) != n or len(tgt) != n:
        raise ValueError("one source and one target set per job")
    src = [np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 6)) for a in src]
    tgt = [np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 6)) for a in tgt]
    recs = (_lib.IcpInput * max(1, n))()
    so = to = 0
    for k in range(n):
        recs[k].status = int(inputs[k].get("status", 0))
        recs[k].src_offset, recs[k].n_src, recs[k].tgt_offset, recs[k].n_tgt = so, len(src[k]), to, len(tgt[k])
        so += len(src[k])
        to += len(tgt[k])
    sp = np.concatenate(src + [np.zeros((1, 6), np.float32)])
    tp = np.concatenate(tgt + [np.zeros((1, 6), np.float32)])
    p = _icp_params(**params)
    res = (_lib.IcpResult * max(1, n))()
    _lib.check(_lib.lib().p2p_icp_batch(ctx.handle, recs, n, sp.ctypes.data, tp.ctypes.data, C.byref(p), res), "p2p_icp_batch")
    return [_icp_result(r) for r in res[:n]]


def refine_depth_batch(ctx: Context, meshes, depths, jobs, inlier_masks: bool = False, **params):
    """The depth refinement of a frame's detections in one call (p2p_refine_depth_batch; icp3d.py:455-491): the ICP inputs of
    icp_inputs_batch, the ICP of icp_batch, the refined pose and the depth score of depth_score_batch at that pose.  depths and jobs
    as in icp_inputs_batch; params as in icp_batch.  Returns one dict per job: status (0, _lib.ICP_SMALL_BBOX / ICP_FEW_POINTS /
    ICP_NONFINITE), R [3, 3] and t [3] (mm: the refined pose, or the job's own when status != 0), icp_pose (4 x 4, metres), iterations,
    pairs, inlier_count, union_count, fcn, ratio (0 when status != 0) and the input record's fields (bbox, t_init, t_adjusted,
    centroid_src, centroid_tgt, n_src, n_tgt); with inlier_masks=True also a bool array [n_jobs, H, W]."""
    depths = [np.ascontiguousarray(d, dtype=np.float32) for d in depths]
    if not depths:
        raise ValueError("refine_depth_batch needs at least one depth image")
    H, W = depths[0].shape
    if any(d.shape != (H, W) for d in depths):
        raise ValueError("all depth images must have the same size")
    for j in jobs:
        if j.get("union_mask") is None or np.shape(j["union_mask"]) != (H, W):
            raise ValueError("every job needs a union_mask of the depth images' size %r" % ((H, W),))
    keep = []
    arr = _depth_jobs(jobs, keep)
    mh = (C.c_void_p * max(1, len(meshes)))(*[m.handle.value for m in meshes])
    dp = (C.c_void_p * len(depths))(*[d.ctypes.data for d in depths])
    p = _icp_params(**params)
    res = (_lib.RefineResult * max(1, len(jobs)))()
    masks = np.zeros((len(jobs), H, W), np.uint8) if inlier_masks else None
    _lib.check(_lib.lib().p2p_refine_depth_batch(ctx.handle, mh, len(meshes), dp, len(depths), arr, len(jobs), H, W, C.byref(p), res,
                                                 masks.ctypes.data if masks is not None else None), "p2p_refine_depth_batch")
    out = []
    for r in res[:len(jobs)]:
        i, c = r.input, _icp_result(r.icp)
        out.append({"status": c["status"], "R": np.array(r.R[:]).reshape(3, 3), "t": np.array(r.t[:]), "icp_pose": c["pose"],
                    "iterations": c["iterations"], "pairs": c["pairs"], "fval_min": c["fval_min"],
                    "inlier_count": int(r.score.inlier_count), "union_count": int(r.score.union_count), "fcn": float(r.score.fcn),
                    "ratio": float(r.score.ratio), "bbox": list(i.bbox), "t_init": np.array(i.t_init[:]),
                    "t_adjusted": np.array(i.t_adjusted[:]), "centroid_src": np.array(i.centroid_src[:]),
                    "centroid_tgt": np.array(i.centroid_tgt[:]), "n_src": int(i.n_src), "n_tgt": int(i.n_tgt)})
    return (out, masks.astype(bool)) if inlier_masks else out


def _refine_record(r):
    i, c = r.input, _icp_result(r.icp)
    return {"status": c["status"], "R": np.array(r.R[:]).reshape(3, 3), "t": np.array(r.t[:]), "icp_pose": c["pose"],
            "iterations": c["iterations"], "pairs": c["pairs"], "fval_min": c["fval_min"],
            "inlier_count": int(r.score.inlier_count), "union_count": int(r.score.union_count), "fcn": float(r.score.fcn),
            "ratio": float(r.score.ratio), "bbox": list(i.bbox), "t_init": np.array(i.t_init[:]),
            "t_adjusted": np.array(i.t_adjusted[:]), "centroid_src": np.array(i.centroid_src[:]),
            "centroid_tgt": np.array(i.centroid_tgt[:]), "n_src": int(i.n_src), "n_tgt": int(i.n_tgt)}


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))


class Rgbd:
    """One image chunk of the RGB-D evaluation on the device (p2p_rgbd, csrc/rgbd.hip): prepared frames, detector masks, the inlier
    masks of the last refine and one occupancy image per frame."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._h = C.c_void_p()
        _lib.check(_lib.lib().p2p_rgbd_create(ctx.handle, C.byref(self._h)), "p2p_rgbd_create")
        self.n_images, self.H, self.W = 0, 0, 0

    def load(self, rgbs, depths, depth_scales, masks, mask_image):
        """rgbs: [H, W, 3] u8 frames; depths: [H, W] uint16 or float32 (all the same dtype); masks: [n, H, W] detector masks (nonzero
        = in), mask_image[m] = frame of mask m."""
        n = len(rgbs)
        rgbs = [np.ascontiguousarray(r, dtype=np.uint8) for r in rgbs]
        dts = {np.asarray(d).dtype for d in depths}
        if dts <= {np.dtype(np.uint16)}:
            code, depths = _lib.DEPTH_U16, [np.ascontiguousarray(d, dtype=np.uint16) for d in depths]
        elif dts <= {np.dtype(np.float32)}:
            code, depths = _lib.DEPTH_F32, [np.ascontiguousarray(d, dtype=np.float32) for d in depths]
        else:
            raise ValueError("depth frames must all be uint16 or all float32, got %r" % sorted(str(d) for d in dts))
        H, W = depths[0].shape if n else (0, 0)
        if any(r.shape != (H, W, 3) for r in rgbs) or any(d.shape != (H, W) for d in depths):
            raise ValueError("every frame must be %r x 3 and every depth %r" % ((H, W), (H, W)))
        m = np.ascontiguousarray(np.asarray(masks) != 0, dtype=np.uint8).reshape(-1, H, W) if len(masks) else np.zeros((0, H, W), np.uint8)
        mi = _i32(mask_image)
        sc = np.ascontiguousarray(depth_scales, dtype=np.float64)
        rp = (C.c_void_p * max(n, 1))(*[r.ctypes.data for r in rgbs])
        dp = (C.c_void_p * max(n, 1))(*[d.ctypes.data for d in depths])
        _lib.check(_lib.lib().p2p_rgbd_load(self._h, rp, dp, code, sc.ctypes.data_as(C.POINTER(C.c_double)), n, H, W,
                                            m.ctypes.data if m.size else None, mi.ctypes.data_as(C.POINTER(C.c_int)), len(m)),
                   "p2p_rgbd_load")
        self.n_images, self.H, self.W = n, H, W

    def image(self, i):
        """Frame i as est_pose_batch / est_pose_submit take a device frame: (pointer, H, W, 'f32')."""
        s = _lib.Image()
        _lib.check(_lib.lib().p2p_rgbd_image(self._h, i, C.byref(s)), "p2p_rgbd_image")
        return (s.data, s.height, s.width, "f32")

    def read(self, i):
        """-> (depth_t [H, W] float32, depth_valid [H, W] bool, frame [H, W, 3] float32) of frame i."""
        d = np.zeros((self.H, self.W), np.float32)
        v = np.zeros((self.H, self.W), np.uint8)
        f = np.zeros((self.H, self.W, 3), np.float32)
        _lib.check(_lib.lib().p2p_rgbd_read(self._h, i, d.ctypes.data, v.ctypes.data, f.ctypes.data), "p2p_rgbd_read")
        return d, v.astype(bool), f

    def refine(self, meshes, jobs, mask_idx, inlier_masks=False, raw=False, **params):
        """jobs: dicts image (frame), mesh, camK, R, t (mm) as in refine_depth_batch, without union_mask; mask_idx[k]: the detector mask
        of job k.  -> (records as refine_depth_batch returns them, union counts [n] int64[, inlier masks [n, H, W] bool]).  raw=True
        returns the _lib.RefineResult array instead of dicts."""
        n = len(jobs)
        jj = [dict(j, union_mask=None) for j in jobs]
        arr = (_lib.RefineJob * max(1, n))()
        for k, j in enumerate(jj):
            J = arr[k]
            J.img_idx, J.mesh_idx = int(j.get("image", 0)), int(j["mesh"])
            J.camK[:] = [float(v) for v in np.asarray(j["camK"], np.float64).reshape(9)]
            J.R[:] = [float(v) for v in np.asarray(j["R"], np.float64).reshape(9)]
            J.t[:] = [float(v) for v in np.asarray(j["t"], np.float64).reshape(3)]
            J.union_mask = None
        mi = _i32(mask_idx) if n else np.zeros(1, np.int32)
        mh = (C.c_void_p * max(1, len(meshes)))(*[m.handle.value for m in meshes])
        p = _icp_params(**params)
        res = (_lib.RefineResult * max(1, n))()
        cnt = np.zeros(max(n, 1), np.int64)
        masks = np.zeros((n, self.H, self.W), np.uint8) if inlier_masks else None
        _lib.check(_lib.lib().p2p_rgbd_refine(self._h, mh, len(meshes), arr, mi.ctypes.data_as(C.POINTER(C.c_int)), n, C.byref(p), res,
                                              cnt.ctypes.data, masks.ctypes.data if masks is not None and n else None), "p2p_rgbd_refine")
        recs = res if raw else [_refine_record(r) for r in res[:n]]
        out = (recs, cnt[:n])
        return out + (masks.astype(bool),) if inlier_masks else out

    def resolve(self, rnd, images, roi_used, inst_pred, host_records=None, host_masks=None):
        """One round of the walk (p2p_rgbd_resolve).  images: per frame a dict targets [obj ids], inst_counts, rois: list of dicts
        obj, score, valid, mask, cands: list of (obj id, ref) with ref a record index or _lib.RGBD_* code.  roi_used / inst_pred:
        flat int32 arrays (rois, targets in image order), updated in place.  host_records: a _lib.RefineResult array (substitutes the
        last refine's records), host_masks: its inlier masks [n, H, W].  -> rows [n_rois, 16]."""
        tgt_off, tobj, tcnt, roi_off, robj, rsc, rval, rmask, coff, cobj, cref = [0], [], [], [0], [], [], [], [], [0], [], []
        for im in images:
            tobj += list(im["targets"]); tcnt += list(im["inst_counts"]); tgt_off.append(len(tobj))
            for r in im["rois"]:
                robj.append(r["obj"]); rsc.append(float(r["score"])); rval.append(1 if r["valid"] else 0); rmask.append(r["mask"])
                for o, ref in r["cands"]:
                    cobj.append(o); cref.append(ref)
                coff.append(len(cobj))
            roi_off.append(len(robj))
        a = [_i32(x) for x in (tgt_off, tobj, tcnt, roi_off, robj)]
        rs = np.ascontiguousarray(rsc, dtype=np.float64)
        b = [_i32(x) for x in (rval, rmask, coff, cobj, cref)]
        nr = len(robj)
        rows = np.zeros((max(nr, 1), _lib.RGBD_ROW), np.float64)
        if roi_used.dtype != np.int32 or inst_pred.dtype != np.int32:
            raise ValueError("roi_used and inst_pred must be int32 arrays")
        hm, n_rec = None, 0
        if host_records is not None:
            n_rec = len(host_records)
            if host_masks is not None:
                hm = np.ascontiguousarray(np.asarray(host_masks) != 0, dtype=np.uint8)
        ptr = lambda x: x.ctypes.data if x.size else None      # noqa: E731
        _lib.check(_lib.lib().p2p_rgbd_resolve(self._h, int(rnd), len(images), *[ptr(x) for x in a], ptr(rs), *[ptr(x) for x in b],
                                               host_records, hm.ctypes.data if hm is not None and hm.size else None, n_rec,
                                               ptr(roi_used), ptr(inst_pred), rows.ctypes.data), "p2p_rgbd_resolve")
        return rows[:nr]

    def close(self):
        if self._h:
            _lib.lib().p2p_rgbd_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
