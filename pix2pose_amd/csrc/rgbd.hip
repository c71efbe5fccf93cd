// RGB-D evaluation of an image chunk (reference tools/5_evaluation_bop_icp3d.py :331-540): frame preparation (:360-370), the union
// masks and refinement of the candidates with their inputs on the device (:455-491), and the two-round walk over the rois that picks
// each roi's best candidate and updates the occupancy image (:394-510).  The rules are in DESIGN.md section 8.3; tests/rgbd_ref.py
// restates them in numpy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "model.h"
#include "pipeline.h"

#pragma clang fp contract(off)     // no FMA contraction: the restatement evaluates the same expressions in the same order

using namespace p2p;

struct p2p_rgbd {
    Ctx* ctx = nullptr;
    int device = 0;                                // kept apart from ctx: the handle may be destroyed after its context
    int n_images = 0, H = 0, W = 0, n_masks = 0;
    std::vector<int> mask_image;
    DevBuf raw, rgb, dt, dv, frame, det;           // chunk: raw depth, u8 RGB, depth_t, depth_valid, float32 frames, detector masks
    DevBuf umask, ucount, jmeta;                   // refine: union masks, their counts, per-job (image, mask) pairs
    DevBuf inl, rec, recmask;                      // refine: inlier masks of the refined jobs, records, record -> inlier mask slot
    int n_rec = 0;
    std::vector<int> recmask_host;
    DevBuf hrec, hmask, hrecmask;                  // resolve: host-supplied records and masks
    DevBuf occ, rin, rout, err;                    // resolve: occupancy [n_images][H][W], packed inputs, rows, error flag
};

namespace {

constexpr int PREP_THREADS = 256, UNION_THREADS = 256, RESOLVE_THREADS = 256;
constexpr int RESOLVE_MAX_TARGETS = 64;        // targets of one image (BOP images have a few to ~20)
constexpr int ROW = 16;                         // obj_id, score, R[9], t[3], round, r_id

// :360-370, one pixel per thread, blockIdx.y = image.  Division and products are correctly rounded float32 (no contraction, no
// reciprocal): depth_t = (raw / 1000) * depth_scale, compared with the float32 thresholds as numpy compares a float32 array with a
// Python float.
template <typename T>
__global__ void __launch_bounds__(PREP_THREADS) prepare_kernel(const T* __restrict__ raw, const unsigned char* __restrict__ rgb,
                                                              const float* __restrict__ scale, size_t HW, float* __restrict__ dt,
                                                              unsigned char* __restrict__ dv, float* __restrict__ frame)
{
    const size_t p = (size_t)blockIdx.x * PREP_THREADS + threadIdx.x;
    if (p >= HW) return;
    const size_t q = (size_t)blockIdx.y * HW + p;
    const float d = __fmul_rn(__fdiv_rn((float)raw[q], 1000.0f), scale[blockIdx.y]);
    const bool valid = d > 0.2f && d < 2.2f;
    const bool zero = isnan(d) || d == 0.0f;        // nan_to_num(depth_t) == 0 (an infinity maps to +-FLT_MAX, not 0)
    const bool keep = valid || zero;
    dt[q] = d;
    dv[q] = valid ? 1 : 0;
    for (int c = 0; c < 3; ++c) {
        const float x = (float)rgb[q * 3 + c];
        frame[q * 3 + c] = keep ? x : __fmul_rn(x, 0.1f);
    }
}

// union_mask = det_mask & depth_valid (:455-456) and its count, blockIdx.y = job.  meta[2 j] = image, meta[2 j + 1] = mask.
__global__ void __launch_bounds__(UNION_THREADS) union_kernel(const unsigned char* __restrict__ det, const unsigned char* __restrict__ dv,
                                                             const int* __restrict__ meta, size_t HW, unsigned char* __restrict__ um,
                                                             unsigned long long* __restrict__ count)
{
    __shared__ unsigned red[UNION_THREADS];
    const int j = blockIdx.y;
    const unsigned char* d = det + (size_t)meta[2 * j + 1] * HW;
    const unsigned char* v = dv + (size_t)meta[2 * j] * HW;
    unsigned char* u = um + (size_t)j * HW;
    unsigned n = 0;
    const size_t chunk = (HW + gridDim.x - 1) / gridDim.x;
    const size_t p0 = blockIdx.x * chunk, p1 = min(HW, p0 + chunk);
    for (size_t p = p0 + threadIdx.x; p < p1; p += UNION_THREADS) {
        const unsigned char b = (d[p] != 0 && v[p] != 0) ? 1 : 0;
        u[p] = b;
        n += b;
    }
    red[threadIdx.x] = n;
    __syncthreads();
    for (int s = UNION_THREADS / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0 && red[0]) atomicAdd(count + j, (unsigned long long)red[0]);     // integer sum: order-independent
}

struct ResolveArgs {
    int round, HW;
    const int *tgt_off, *target_obj, *inst_count, *roi_off, *roi_obj, *roi_valid, *roi_mask, *cand_off, *cand_obj, *cand_ref;
    const double* roi_score;
    const p2p_refine_result* rec;
    const int* rec_mask;                       // record -> inlier mask slot, -1 = all zero
    const unsigned char* inl;                  // inlier masks [slot][H][W]
    const unsigned char* det;                  // detector masks [m][H][W]
    unsigned char* occ;                        // [image][H][W], 0 / 1 (the reference's bool occupancy)
    int *roi_used, *inst_pred;
    double* rows;
    int* err;
};

// One workgroup walks one image's rois in order (:394-510).  Thread 0 holds the control flow; the workgroup counts the IoU of the
// occupancy with the roi's detector mask (integer counts, one float64 division as numpy's ratio of two integer sums) and applies the
// occupancy update.
__global__ void __launch_bounds__(RESOLVE_THREADS) resolve_kernel(ResolveArgs a)
{
    __shared__ unsigned long long s_in[RESOLVE_THREADS], s_un[RESOLVE_THREADS];
    __shared__ int s_mode, s_stop, s_nc, s_upd, s_mask;
    __shared__ int s_cobj[RESOLVE_MAX_TARGETS], s_cg[RESOLVE_MAX_TARGETS];
    const int img = blockIdx.x, tid = threadIdx.x;
    const size_t HW = (size_t)a.HW;
    unsigned char* occ = a.occ + (size_t)img * HW;
    const int t0 = a.tgt_off[img], nt = a.tgt_off[img + 1] - t0;
    for (int r = a.roi_off[img]; r < a.roi_off[img + 1]; ++r) {
        if (tid == 0) {
            s_mode = -1;      // -1 skip the roi, 0 IoU against an empty occupancy, 1 against the occupancy
            s_stop = 0;
            s_nc = 0;
            if (a.round == 1 && a.roi_used[r]) {
            } else if (!a.roi_valid[r]) {
            } else if (a.round == 0) {
                const int obj = a.roi_obj[r];
                int g = -1;
                for (int k = 0; k < nt && g < 0; ++k)
                    if (a.target_obj[t0 + k] == obj) g = k;
                if (g >= 0) {
                    s_mode = obj == 1 ? 1 : 0;     // occupancy == obj_id on a bool image: the occupancy itself for obj 1, empty otherwise
                    s_cobj[0] = obj;
                    s_cg[0] = g;
                    s_nc = 1;
                }
            } else {
                int nc = 0;                        // the missing objects, recomputed at every roi (:419-428)
                for (int k = 0; k < nt; ++k)
                    if (a.inst_pred[t0 + k] < a.inst_count[t0 + k]) {
                        s_cobj[nc] = a.target_obj[t0 + k];
                        s_cg[nc] = k;
                        ++nc;
                    }
                s_nc = nc;
                if (nc == 0) s_stop = 1;
                else s_mode = 1;                    // occupancy != 0
            }
            s_mask = a.roi_mask[r];
        }
        __syncthreads();
        if (s_stop) break;
        if (s_mode >= 0) {
            const unsigned char* d = a.det + (size_t)s_mask * HW;
            unsigned long long ni = 0, nu = 0;
            for (size_t p = tid; p < HW; p += RESOLVE_THREADS) {
                const bool o = s_mode == 1 && occ[p] != 0, m = d[p] != 0;
                ni += (o && m) ? 1 : 0;
                nu += (o || m) ? 1 : 0;
            }
            s_in[tid] = ni;
            s_un[tid] = nu;
            __syncthreads();
            for (int s = RESOLVE_THREADS / 2; s > 0; s >>= 1) {
                if (tid < s) { s_in[tid] += s_in[tid + s]; s_un[tid] += s_un[tid + s]; }
                __syncthreads();
            }
            if (tid == 0) {
                s_upd = -1;
                const double iou = (double)s_in[0] / (double)s_un[0];      // 0 / 0 is NaN and does not skip
                if (!(iou > 0.7)) {
                    double best = 0.0, best_ratio = 0.0;
                    int best_obj = 0, best_g = 0, best_rec = -1, last = -1;
                    for (int c = 0; c < s_nc; ++c) {
                        const int obj = s_cobj[c];
                        int ref = P2P_RGBD_NOT_EVALUATED;
                        bool found = false;
                        for (int q = a.cand_off[r]; q < a.cand_off[r + 1] && !found; ++q)
                            if (a.cand_obj[q] == obj) { ref = a.cand_ref[q]; found = true; }
                        if (ref == P2P_RGBD_NOT_EVALUATED) { atomicOr(a.err, 1); continue; }
                        if (ref < 0) continue;                               // est_pose failed, or t_z < 0.2 m
                        const p2p_refine_result& R = a.rec[ref];
                        if (R.icp.status != 0) continue;                     // union <= 30, or the ICP's -1
                        const double score = (a.round == 0 ? a.roi_score[r] : 0.001) * R.score.fcn;
                        last = ref;                                          // inlier_mask of :476: the last scored candidate's
                        if (best < score) {
                            best = score; best_obj = obj; best_g = s_cg[c]; best_ratio = R.score.ratio; best_rec = ref;
                        }
                    }
                    if (best > 0.0) {
                        if (a.round == 0 || best_ratio > 0.5) {
                            a.inst_pred[t0 + best_g] += 1;
                            a.roi_used[r] = 1;
                            s_upd = a.rec_mask[last];
                        }
                        double* row = a.rows + (size_t)r * ROW;
                        const p2p_refine_result& B = a.rec[best_rec];
                        row[0] = best_obj;
                        row[1] = best;
                        for (int k = 0; k < 9; ++k) row[2 + k] = B.R[k];
                        for (int k = 0; k < 3; ++k) row[11 + k] = B.t[k];
                        row[14] = a.round;
                        row[15] = r - a.roi_off[img];
                    }
                }
            }
            __syncthreads();
            if (s_upd >= 0) {                                                // occupancy[inlier_mask] = best_obj_id (> 0: True)
                const unsigned char* m = a.inl + (size_t)s_upd * HW;
                for (size_t p = tid; p < HW; p += RESOLVE_THREADS)
                    if (m[p]) occ[p] = 1;
            }
        }
        __syncthreads();
    }
}

int upload(DevBuf& b, const void* src, size_t bytes, hipStream_t st)
{
    int rc = b.reserve(std::max<size_t>(bytes, 1));
    if (rc) return rc;
    if (bytes) HIP_TRY(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st));
    return P2P_OK;
}

}  // namespace

extern "C" {

int p2p_rgbd_create(p2p_ctx* ctx, p2p_rgbd** out)
{
    if (!ctx || !out) {
        set_error("p2p_rgbd_create: bad arguments");
        return P2P_ERR_INVALID_ARG;
    }
    p2p_rgbd* h = new (std::nothrow) p2p_rgbd;
    if (!h) {
        set_error("p2p_rgbd_create: out of host memory");
        return P2P_ERR_HIP;
    }
    h->ctx = reinterpret_cast<Ctx*>(ctx);
    h->device = h->ctx->device;
    *out = h;
    return P2P_OK;
}

void p2p_rgbd_destroy(p2p_rgbd* h)
{
    if (!h) return;
    hipSetDevice(h->device);           // the buffers' hipFree waits for the work that reads them; the context itself may be gone already
    delete h;
}

int p2p_rgbd_load(p2p_rgbd* h, const unsigned char* const* rgb, const void* const* depth, int depth_dtype, const double* depth_scale,
                  int n_images, int height, int width, const unsigned char* masks, const int* mask_image, int n_masks)
{
    const char* who = "p2p_rgbd_load";
    if (!h || n_images < 1 || n_masks < 0 || !rgb || !depth || !depth_scale || (n_masks > 0 && (!masks || !mask_image)) ||
        (depth_dtype != P2P_DEPTH_U16 && depth_dtype != P2P_DEPTH_F32) || height <= 0 || width <= 0 ||
        (int64_t)height * width > (1 << 26)) {
        set_error("%s: bad arguments", who);
        return P2P_ERR_INVALID_ARG;
    }
    for (int i = 0; i < n_images; ++i)
        if (!rgb[i] || !depth[i]) {
            set_error("%s: frame %d is null", who, i);
            return P2P_ERR_INVALID_ARG;
        }
    for (int m = 0; m < n_masks; ++m)
        if (mask_image[m] < 0 || mask_image[m] >= n_images) {
            set_error("%s: mask %d names frame %d of %d", who, m, mask_image[m], n_images);
            return P2P_ERR_INVALID_ARG;
        }
    Ctx& X = *h->ctx;
    HIP_TRY(hipSetDevice(X.device));
    hipStream_t st = X.stream;
    HIP_TRY(hipStreamSynchronize(st));           // queued work of the previous chunk may still read the buffers
    const size_t HW = (size_t)height * width, esz = depth_dtype == P2P_DEPTH_U16 ? 2 : 4;
    int rc;
    h->n_images = 0;
    h->n_rec = 0;
    if ((rc = h->raw.reserve(n_images * HW * esz)) || (rc = h->rgb.reserve(n_images * HW * 3)) || (rc = h->dt.reserve(n_images * HW * 4)) ||
        (rc = h->dv.reserve(n_images * HW)) || (rc = h->frame.reserve(n_images * HW * 12)) ||
        (rc = h->det.reserve(std::max<size_t>(n_masks * HW, 1))) || (rc = h->occ.reserve(n_images * HW)))
        return rc;
    std::vector<float> sc(n_images);
    for (int i = 0; i < n_images; ++i) {
        sc[i] = (float)depth_scale[i];             // numpy: float32 array * Python float -> the float is taken as float32
        HIP_TRY(hipMemcpyAsync(h->raw.as<char>() + i * HW * esz, depth[i], HW * esz, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(h->rgb.as<unsigned char>() + i * HW * 3, rgb[i], HW * 3, hipMemcpyHostToDevice, st));
    }
    if (n_masks) HIP_TRY(hipMemcpyAsync(h->det.p, masks, n_masks * HW, hipMemcpyHostToDevice, st));
    DevBuf dsc;
    if ((rc = dsc.reserve(sizeof(float) * n_images))) return rc;
    HIP_TRY(hipMemcpyAsync(dsc.p, sc.data(), sizeof(float) * n_images, hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)((HW + PREP_THREADS - 1) / PREP_THREADS), n_images);
    if (depth_dtype == P2P_DEPTH_U16)
        prepare_kernel<unsigned short><<<grid, PREP_THREADS, 0, st>>>(h->raw.as<unsigned short>(), h->rgb.as<unsigned char>(),
                                                                    dsc.as<float>(), HW, h->dt.as<float>(), h->dv.as<unsigned char>(),
                                                                    h->frame.as<float>());
    else
        prepare_kernel<float><<<grid, PREP_THREADS, 0, st>>>(h->raw.as<float>(), h->rgb.as<unsigned char>(), dsc.as<float>(), HW,
                                                           h->dt.as<float>(), h->dv.as<unsigned char>(), h->frame.as<float>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    h->n_images = n_images;
    h->H = height;
    h->W = width;
    h->n_masks = n_masks;
    h->mask_image.assign(mask_image, mask_image + n_masks);
    return P2P_OK;
}

int p2p_rgbd_image(p2p_rgbd* h, int i, p2p_image* out)
{
    if (!h || !out || i < 0 || i >= h->n_images) {
        set_error("p2p_rgbd_image: bad arguments");
        return P2P_ERR_INVALID_ARG;
    }
    out->data = h->frame.as<float>() + (size_t)i * h->H * h->W * 3;
    out->height = h->H;
    out->width = h->W;
    out->dtype = P2P_IMG_F32;
    out->mem = P2P_MEM_DEVICE;
    return P2P_OK;
}

int p2p_rgbd_read(p2p_rgbd* h, int i, float* depth_t, unsigned char* depth_valid, float* frame)
{
    if (!h || i < 0 || i >= h->n_images) {
        set_error("p2p_rgbd_read: bad arguments");
        return P2P_ERR_INVALID_ARG;
    }
    Ctx& X = *h->ctx;
    HIP_TRY(hipSetDevice(X.device));
    const size_t HW = (size_t)h->H * h->W;
    if (depth_t) HIP_TRY(hipMemcpyAsync(depth_t, h->dt.as<float>() + i * HW, HW * 4, hipMemcpyDeviceToHost, X.stream));
    if (depth_valid) HIP_TRY(hipMemcpyAsync(depth_valid, h->dv.as<unsigned char>() + i * HW, HW, hipMemcpyDeviceToHost, X.stream));
    if (frame) HIP_TRY(hipMemcpyAsync(frame, h->frame.as<float>() + i * HW * 3, HW * 12, hipMemcpyDeviceToHost, X.stream));
    HIP_TRY(hipStreamSynchronize(X.stream));
    return P2P_OK;
}

int p2p_rgbd_refine(p2p_rgbd* h, const p2p_mesh* const* meshes, int n_meshes, const p2p_refine_job* jobs, const int* mask_idx, int n_jobs,
                    const p2p_icp_params* params, p2p_refine_result* out, int64_t* union_counts, unsigned char* inlier_masks)
{
    const char* who = "p2p_rgbd_refine";
    if (!h || h->n_images == 0 || n_jobs < 0 || n_jobs > 65535 || (n_jobs > 0 && (!jobs || !mask_idx || !out || !union_counts))) {
        set_error("%s: bad arguments (or no chunk loaded)", who);
        return P2P_ERR_INVALID_ARG;
    }
    for (int j = 0; j < n_jobs; ++j) {
        const int m = mask_idx[j], im = jobs[j].img_idx;
        if (im < 0 || im >= h->n_images || m < 0 || m >= h->n_masks || h->mask_image[m] != im) {
            set_error("%s: job %d: frame %d of %d, mask %d of %d", who, j, im, h->n_images, m, h->n_masks);
            return P2P_ERR_INVALID_ARG;
        }
    }
    Ctx& X = *h->ctx;
    HIP_TRY(hipSetDevice(X.device));
    hipStream_t st = X.stream;
    const size_t HW = (size_t)h->H * h->W;
    h->n_rec = 0;
    int rc;
    std::vector<int> meta(2 * std::max(n_jobs, 1));
    for (int j = 0; j < n_jobs; ++j) { meta[2 * j] = jobs[j].img_idx; meta[2 * j + 1] = mask_idx[j]; }
    std::vector<unsigned long long> cnt(std::max(n_jobs, 1), 0);
    if (n_jobs > 0) {
        if ((rc = h->umask.reserve(n_jobs * HW)) || (rc = h->ucount.reserve(8 * n_jobs)) ||
            (rc = upload(h->jmeta, meta.data(), sizeof(int) * 2 * n_jobs, st)))
            return rc;
        HIP_TRY(hipMemsetAsync(h->ucount.p, 0, 8 * n_jobs, st));
        const unsigned bx = (unsigned)std::min<size_t>(64, (HW + UNION_THREADS * 16 - 1) / (UNION_THREADS * 16));
        union_kernel<<<dim3(bx, n_jobs), UNION_THREADS, 0, st>>>(h->det.as<unsigned char>(), h->dv.as<unsigned char>(), h->jmeta.as<int>(),
                                                                 HW, h->umask.as<unsigned char>(), h->ucount.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(cnt.data(), h->ucount.p, 8 * n_jobs, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    // the union gate (:457-459) before the ICP; the rest go through the chain of p2p_refine_depth_batch on device inputs
    std::vector<p2p_refine_job> sub;
    std::vector<int> sub_of;
    for (int j = 0; j < n_jobs; ++j) {
        union_counts[j] = (int64_t)cnt[j];
        if (cnt[j] > 30) {
            p2p_refine_job J = jobs[j];
            J.union_mask = h->umask.as<unsigned char>() + j * HW;
            sub.push_back(J);
            sub_of.push_back(j);
        }
    }
    const int ns = (int)sub.size();
    std::vector<const float*> dimg(h->n_images);
    for (int i = 0; i < h->n_images; ++i) dimg[i] = h->dt.as<float>() + i * HW;
    std::vector<p2p_refine_result> sres(std::max(ns, 1));
    if (ns > 0 &&
        (rc = refine_chain(who, reinterpret_cast<p2p_ctx*>(&X), meshes, n_meshes, dimg.data(), h->n_images, sub.data(), ns, h->H, h->W,
                           params, sres.data(), nullptr, true, &h->inl)))
        return rc;
    h->recmask_host.assign(std::max(n_jobs, 1), -1);
    for (int j = 0; j < n_jobs; ++j) {
        p2p_refine_result& R = out[j];
        std::memset(&R, 0, sizeof(R));
        R.input.status = R.icp.status = P2P_RGBD_SMALL_UNION;
        for (int k = 0; k < 4; ++k) R.icp.pose[5 * k] = 1.0;
        for (int k = 0; k < 9; ++k) R.R[k] = jobs[j].R[k];
        for (int k = 0; k < 3; ++k) R.t[k] = jobs[j].t[k];
    }
    for (int k = 0; k < ns; ++k) {
        out[sub_of[k]] = sres[k];
        h->recmask_host[sub_of[k]] = k;
    }
    if (n_jobs > 0) {
        if ((rc = upload(h->rec, out, sizeof(p2p_refine_result) * n_jobs, st)) ||
            (rc = upload(h->recmask, h->recmask_host.data(), sizeof(int) * n_jobs, st)))
            return rc;
        if (inlier_masks) {
            for (int j = 0; j < n_jobs; ++j) {
                const int k = h->recmask_host[j];
                if (k >= 0) HIP_TRY(hipMemcpyAsync(inlier_masks + j * HW, h->inl.as<unsigned char>() + k * HW, HW, hipMemcpyDeviceToHost, st));
                else std::memset(inlier_masks + j * HW, 0, HW);
            }
        }
        HIP_TRY(hipStreamSynchronize(st));
    }
    h->n_rec = n_jobs;
    return P2P_OK;
}

int p2p_rgbd_resolve(p2p_rgbd* h, int round, int n_images, const int* tgt_off, const int* target_obj, const int* inst_count,
                     const int* roi_off, const int* roi_obj, const double* roi_score, const int* roi_valid, const int* roi_mask,
                     const int* cand_off, const int* cand_obj, const int* cand_ref, const p2p_refine_result* host_records,
                     const unsigned char* host_masks, int n_records, int* roi_used, int* inst_pred, double* rows)
{
    const char* who = "p2p_rgbd_resolve";
    if (!h || (round != 0 && round != 1) || n_images != h->n_images || n_images < 1 || !tgt_off || !roi_off || !cand_off ||
        !roi_used || !inst_pred || !rows || (host_records && n_records < 0)) {
        set_error("%s: bad arguments (n_images must be the loaded chunk's %d)", who, h ? h->n_images : 0);
        return P2P_ERR_INVALID_ARG;
    }
    const int nt = tgt_off[n_images], nr = roi_off[n_images];
    if (tgt_off[0] != 0 || roi_off[0] != 0 || nt < 0 || nr < 0) {
        set_error("%s: offsets must start at 0", who);
        return P2P_ERR_INVALID_ARG;
    }
    for (int i = 0; i < n_images; ++i)
        if (tgt_off[i + 1] < tgt_off[i] || tgt_off[i + 1] - tgt_off[i] > RESOLVE_MAX_TARGETS || roi_off[i + 1] < roi_off[i]) {
            set_error("%s: image %d: bad offsets or more than %d targets", who, i, RESOLVE_MAX_TARGETS);
            return P2P_ERR_INVALID_ARG;
        }
    if ((nt > 0 && (!target_obj || !inst_count)) || (nr > 0 && (!roi_obj || !roi_score || !roi_valid || !roi_mask))) {
        set_error("%s: null array", who);
        return P2P_ERR_INVALID_ARG;
    }
    if (cand_off[0] != 0) {
        set_error("%s: offsets must start at 0", who);
        return P2P_ERR_INVALID_ARG;
    }
    for (int r = 0; r < nr; ++r)
        if (cand_off[r + 1] < cand_off[r]) {
            set_error("%s: bad candidate offsets at roi %d", who, r);
            return P2P_ERR_INVALID_ARG;
        }
    const int nc = cand_off[nr];
    if (nc > 0 && (!cand_obj || !cand_ref)) {
        set_error("%s: null candidate array", who);
        return P2P_ERR_INVALID_ARG;
    }
    const int n_rec = host_records ? n_records : h->n_rec;
    for (int q = 0; q < nc; ++q)
        if (cand_ref[q] >= n_rec || cand_ref[q] < P2P_RGBD_NEAR) {
            set_error("%s: candidate %d names record %d of %d", who, q, cand_ref[q], n_rec);
            return P2P_ERR_INVALID_ARG;
        }
    for (int i = 0; i < n_images; ++i)
        for (int r = roi_off[i]; r < roi_off[i + 1]; ++r)
            if (roi_valid[r] && (roi_mask[r] < 0 || roi_mask[r] >= h->n_masks || h->mask_image[roi_mask[r]] != i)) {
                set_error("%s: roi %d names mask %d of %d (or another frame's)", who, r, roi_mask[r], h->n_masks);
                return P2P_ERR_INVALID_ARG;
            }
    Ctx& X = *h->ctx;
    HIP_TRY(hipSetDevice(X.device));
    hipStream_t st = X.stream;
    const size_t HW = (size_t)h->H * h->W;
    int rc;
    // packed int inputs: tgt_off, target_obj, inst_count, roi_off, roi_obj, roi_valid, roi_mask, cand_off, cand_obj, cand_ref,
    // roi_used, inst_pred; then roi_score (double) in its own buffer
    std::vector<int> pk;
    std::vector<size_t> at;
    auto put = [&](const int* p, int n) { at.push_back(pk.size()); if (n > 0) pk.insert(pk.end(), p, p + n); };
    put(tgt_off, n_images + 1); put(target_obj, nt); put(inst_count, nt); put(roi_off, n_images + 1); put(roi_obj, nr); put(roi_valid, nr);
    put(roi_mask, nr); put(cand_off, nr + 1); put(cand_obj, nc); put(cand_ref, nc); put(roi_used, nr); put(inst_pred, nt);
    const size_t nint = pk.size();
    const size_t sbytes = ((sizeof(int) * nint + 15) / 16) * 16;
    if ((rc = h->rin.reserve(sbytes + sizeof(double) * std::max(nr, 1))) || (rc = h->rout.reserve(sizeof(double) * ROW * std::max(nr, 1))) ||
        (rc = h->err.reserve(sizeof(int))))
        return rc;
    HIP_TRY(hipMemcpyAsync(h->rin.p, pk.data(), sizeof(int) * nint, hipMemcpyHostToDevice, st));
    if (nr) HIP_TRY(hipMemcpyAsync(h->rin.as<char>() + sbytes, roi_score, sizeof(double) * nr, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(h->rout.p, 0, sizeof(double) * ROW * std::max(nr, 1), st));
    HIP_TRY(hipMemsetAsync(h->err.p, 0, sizeof(int), st));
    if (round == 0) HIP_TRY(hipMemsetAsync(h->occ.p, 0, n_images * HW, st));
    const p2p_refine_result* rec = h->rec.as<p2p_refine_result>();
    const int* recmask = h->recmask.as<int>();
    const unsigned char* inl = h->inl.as<unsigned char>();
    if (host_records) {
        std::vector<int> rm(std::max(n_records, 1));
        for (int k = 0; k < n_records; ++k) rm[k] = host_masks ? k : -1;
        if ((rc = upload(h->hrec, host_records, sizeof(p2p_refine_result) * n_records, st)) ||
            (rc = upload(h->hrecmask, rm.data(), sizeof(int) * n_records, st)) ||
            (host_masks && (rc = upload(h->hmask, host_masks, n_records * HW, st))))
            return rc;
        HIP_TRY(hipStreamSynchronize(st));       // rm is a local
        rec = h->hrec.as<p2p_refine_result>();
        recmask = h->hrecmask.as<int>();
        inl = h->hmask.as<unsigned char>();
    }
    ResolveArgs a;
    const int* base = h->rin.as<int>();
    a.round = round;
    a.HW = (int)HW;
    a.tgt_off = base + at[0]; a.target_obj = base + at[1]; a.inst_count = base + at[2]; a.roi_off = base + at[3];
    a.roi_obj = base + at[4]; a.roi_valid = base + at[5]; a.roi_mask = base + at[6]; a.cand_off = base + at[7];
    a.cand_obj = base + at[8]; a.cand_ref = base + at[9];
    a.roi_used = const_cast<int*>(base) + at[10];
    a.inst_pred = const_cast<int*>(base) + at[11];
    a.roi_score = reinterpret_cast<const double*>(h->rin.as<char>() + sbytes);
    a.rec = rec; a.rec_mask = recmask; a.inl = inl;
    a.det = h->det.as<unsigned char>();
    a.occ = h->occ.as<unsigned char>();
    a.rows = h->rout.as<double>();
    a.err = h->err.as<int>();
    resolve_kernel<<<n_images, RESOLVE_THREADS, 0, st>>>(a);
    HIP_TRY(hipGetLastError());
    int err = 0;
    std::vector<int> back(nint);
    HIP_TRY(hipMemcpyAsync(back.data(), h->rin.p, sizeof(int) * nint, hipMemcpyDeviceToHost, st));
    if (nr) HIP_TRY(hipMemcpyAsync(rows, h->rout.p, sizeof(double) * ROW * nr, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&err, h->err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (nr) std::memcpy(roi_used, back.data() + at[10], sizeof(int) * nr);
    if (nt) std::memcpy(inst_pred, back.data() + at[11], sizeof(int) * nt);
    if (err) {
        set_error("%s: the walk reached a candidate that was not evaluated", who);
        return P2P_ERR_INVALID_ARG;
    }
    return P2P_OK;
}

}  // extern "C"
