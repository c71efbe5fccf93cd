// Depth back-projection, surface normals and the point sets of the ICP refinement (reference pix2pose_util/common_util.py getXYZ :13-30,
// get_normal(refine=True) :32-89, get_bbox_from_mask :5-10, and tools/5_evaluation_bop_icp3d.py :372-374, :464, icp_refinement :58-85).
// The rules (int16 pixel offsets, the onion-peel stand-in for cv2.inpaint, scipy's Gaussian, numpy's gradient, the bbox quirk, the
// gates and the centroid shift) are written down in DESIGN.md section 8; tests/normals_ref.py restates them in float64 numpy.
//
// One "item" is an image whose normals are wanted over a crop: a whole sensor frame (crop = frame), or the rendered depth of one ICP job
// (crop = the bbox of its init_mask).  Fill and Gaussian run over the item's work region: the whole frame, or for a job its crop grown by
// NRM_GROW and clipped to the frame, which gives the same bits at every crop pixel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels.h"
#include "model.h"
#include "pipeline.h"

#pragma clang fp contract(off)     // no FMA contraction: the restatement evaluates the same expressions in the same order

namespace p2p {

namespace {

constexpr int FILL_LAYERS = 10;                   // L of the onion-peel fill; outputs at d > 0 do not depend on it once L >= 10
constexpr int GAUSS_R = 8;                        // ndimage.gaussian_filter(., 2): truncate 4.0 -> radius 8
constexpr int NRM_GROW = GAUSS_R + 2 * FILL_LAYERS;   // crop -> work region of a job (a filled value reads 2 px per layer)
constexpr int MAX_SIDE = 16384;                   // keeps every int16 pixel offset of the reference in range (|cx|, |cy| < MAX_SIDE too)
constexpr int TX = 64, TY = 4;                    // per-pixel kernels: one wave per row segment

struct NrmItem {
    const float* depth;                 // raw depth [H][W] of the frame (sensor image, or the job's z-buffer)
    const unsigned char* umask;         // jobs: union mask [H][W] (nonzero = in); null for frames
    int r0, c0, rh, rw;                 // work region in frame pixels
    int g0, gc0, gh, gw;                // gradient crop in frame pixels, inside the region
    double fx, fy, cx, cy;
    float* fa;                          // [rh][rw] fill ping-pong (NaN = unknown)
    float* fb;
    double* tmp;                        // [rh][rw] after the first Gaussian pass (axis 0)
    double* sm;                         // [rh][rw] smoothed depth
    float* pts;                         // [gh][gw][6] x y z nx ny nz
    unsigned char* cmask;               // jobs: init_mask over the crop [gh][gw]; null for frames
};

// numpy's nan_to_num on float32: NaN -> 0, +-inf -> +-FLT_MAX
__device__ __forceinline__ float nan_to_num_f(float v)
{
    if (isnan(v)) return 0.0f;
    if (isinf(v)) return v > 0.0f ? 3.402823466e+38f : -3.402823466e+38f;
    return v;
}
// nan_to_num of a normal component: c / |c| is NaN or within [-1, 1], never infinite
__device__ __forceinline__ double nan_to_num_d(double v) { return isnan(v) ? 0.0 : v; }

// scipy's 'reflect' extension (d c b a | a b c d), repeated for lines shorter than the radius: period 2n
__device__ __forceinline__ int reflect_idx(int i, int n)
{
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m >= n ? p - 1 - m : m;
}

// Layer 0 of the fill: the known pixels are those with nan_to_num(d) != 0, the rest are marked unknown (NaN).
__global__ void __launch_bounds__(TX * TY) fill_init_kernel(const NrmItem* __restrict__ items, int W)
{
    const NrmItem& I = items[blockIdx.z];
    const int c = blockIdx.x * TX + threadIdx.x, r = blockIdx.y * TY + threadIdx.y;
    if (r >= I.rh || c >= I.rw) return;
    const float v = nan_to_num_f(I.depth[(size_t)(I.r0 + r) * W + I.c0 + c]);
    I.fa[(size_t)r * I.rw + c] = v != 0.0f ? v : __int_as_float(0x7fc00000);
}

// One onion-peel layer: an unknown pixel with a known 8-neighbour gets the mean of the known pixels of its 5 x 5 window (float64 sum in
// row-major window order, rounded to float32).  Known and unknown are those of the previous layer; the window is clipped to the region.
__global__ void __launch_bounds__(TX * TY) fill_layer_kernel(const NrmItem* __restrict__ items, int parity)
{
    const NrmItem& I = items[blockIdx.z];
    const int c = blockIdx.x * TX + threadIdx.x, r = blockIdx.y * TY + threadIdx.y;
    if (r >= I.rh || c >= I.rw) return;
    const float* src = parity ? I.fb : I.fa;
    float* dst = parity ? I.fa : I.fb;
    const size_t rw = I.rw;
    const float v = src[r * rw + c];
    if (!isnan(v)) {
        dst[r * rw + c] = v;
        return;
    }
    bool near = false;
    for (int dr = -1; dr <= 1; ++dr)
        for (int dc = -1; dc <= 1; ++dc) {
            const int rr = r + dr, cc = c + dc;
            if (rr >= 0 && rr < I.rh && cc >= 0 && cc < I.rw && !isnan(src[rr * rw + cc])) near = true;
        }
    float out = __int_as_float(0x7fc00000);
    if (near) {
        double s = 0.0;
        int n = 0;
        for (int dr = -2; dr <= 2; ++dr)
            for (int dc = -2; dc <= 2; ++dc) {
                const int rr = r + dr, cc = c + dc;
                if (rr < 0 || rr >= I.rh || cc < 0 || cc >= I.rw) continue;
                const float w = src[rr * rw + cc];
                if (!isnan(w)) { s += (double)w; ++n; }
            }
        out = (float)(s / (double)n);
    }
    dst[r * rw + c] = out;
}

struct GaussW {
    double w[GAUSS_R + 1];              // centre first
};

// ndimage.correlate1d's symmetric loop: x[0] w[0], then (x[-k] + x[+k]) w[k] for k = R .. 1.  Indices reflect at the FRAME border; a
// reflected index outside the region is clamped into it (only pixels no crop pixel reads are affected).
template <int AXIS>
__global__ void __launch_bounds__(TX * TY) gauss_kernel(const NrmItem* __restrict__ items, int H, int W, GaussW g, int final_parity)
{
    const NrmItem& I = items[blockIdx.z];
    const int c = blockIdx.x * TX + threadIdx.x, r = blockIdx.y * TY + threadIdx.y;
    if (r >= I.rh || c >= I.rw) return;
    const size_t rw = I.rw;
    double x0, acc;
    if (AXIS == 0) {
        const float* f = final_parity ? I.fb : I.fa;
        auto at = [&](int k) -> double {
            int rr = reflect_idx(I.r0 + r + k, H) - I.r0;
            rr = min(max(rr, 0), I.rh - 1);
            const float v = f[rr * rw + c];
            return isnan(v) ? 0.0 : (double)v;          // still unknown after the last layer: 0
        };
        x0 = at(0);
        acc = x0 * g.w[0];
        for (int k = GAUSS_R; k >= 1; --k) acc += (at(-k) + at(k)) * g.w[k];
        I.tmp[r * rw + c] = acc;
    } else {
        auto at = [&](int k) -> double {
            int cc = reflect_idx(I.c0 + c + k, W) - I.c0;
            cc = min(max(cc, 0), I.rw - 1);
            return I.tmp[r * rw + cc];
        };
        x0 = at(0);
        acc = x0 * g.w[0];
        for (int k = GAUSS_R; k >= 1; --k) acc += (at(-k) + at(k)) * g.w[k];
        I.sm[r * rw + c] = acc;
    }
}

// np.gradient(f, 2, edge_order=2) along one axis of the crop, at index i of n (n >= 3)
__device__ __forceinline__ double grad2(double fm2, double fm1, double f0, double fp1, double fp2, int i, int n)
{
    if (i == 0) return -0.75 * f0 + 1.0 * fp1 + -0.25 * fp2;
    if (i == n - 1) return 0.25 * fm2 + -1.0 * fm1 + 0.75 * f0;
    return (fp1 - fm1) / 4.0;
}

// Gradient over the crop, normal (get_normal :70-88), back-projection (getXYZ), and for jobs the init_mask over the crop.
__global__ void __launch_bounds__(TX * TY) normal_kernel(const NrmItem* __restrict__ items, int W)
{
    const NrmItem& I = items[blockIdx.z];
    const int j = blockIdx.x * TX + threadIdx.x, i = blockIdx.y * TY + threadIdx.y;
    if (i >= I.gh || j >= I.gw) return;
    const size_t rw = I.rw;
    const int R = I.g0 + i, Cc = I.gc0 + j;                 // frame pixel
    const int lr = R - I.r0, lc = Cc - I.c0;                 // region pixel
    auto S = [&](int di, int dj) -> double {                 // smoothed depth at crop offset (di, dj), clamped to the crop
        const int ii = min(max(i + di, 0), I.gh - 1), jj = min(max(j + dj, 0), I.gw - 1);
        return I.sm[(size_t)(lr + ii - i) * rw + (lc + jj - j)];
    };
    const double s = S(0, 0);
    const double gy = grad2(S(-2, 0), S(-1, 0), s, S(1, 0), S(2, 0), i, I.gh);
    const double gx = grad2(S(0, -2), S(0, -1), s, S(0, 1), S(0, 2), j, I.gw);
    const double uu = (double)(int)((double)Cc - I.cx);     // int16 uv_table: truncated toward zero
    const double uv = (double)(int)((double)R - I.cy);
    const double kx = 1.0 / I.fx, ky = 1.0 / I.fy;
    const double vy0 = uu * kx * gy, vy1 = s * ky + uv * ky * gy, vy2 = gy;
    const double vx0 = s * kx + uu * kx * gx, vx1 = uv * ky * gx, vx2 = gx;
    const double c0 = vx1 * vy2 - vx2 * vy1, c1 = vx2 * vy0 - vx0 * vy2, c2 = vx0 * vy1 - vx1 * vy0;
    double nrm = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
    if (nrm == 0.0) nrm = 1.0;
    const float d = I.depth[(size_t)R * W + Cc];
    float* o = I.pts + ((size_t)i * I.gw + j) * 6;
    o[0] = (float)(uu * (double)d / I.fx);
    o[1] = (float)(uv * (double)d / I.fy);
    o[2] = d;
    o[3] = (float)nan_to_num_d(c0 / nrm);
    o[4] = (float)nan_to_num_d(c1 / nrm);
    o[5] = (float)nan_to_num_d(c2 / nrm);
    if (I.cmask) I.cmask[(size_t)i * I.gw + j] = d > 0.0f && I.umask[(size_t)R * W + Cc] != 0;
}

// Row-major compaction of the [rows][cols][6] points where mask != 0.  Counts per row, an exclusive scan per item in row order, then
// each row writes at its offset with a wave prefix: the order is numpy's boolean-index order, with no atomics.
struct CmpItem {
    const float* pts;
    const unsigned char* mask;
    int rows, cols;
    int64_t row_base;                   // first entry of the item in the per-row count array
    float* out;                         // [n][6]
    int64_t n;                          // points written (filled in by cmp_scan_kernel)
};

__global__ void __launch_bounds__(64) cmp_count_kernel(const CmpItem* __restrict__ items, int64_t* __restrict__ rowcnt)
{
    const CmpItem& I = items[blockIdx.y];
    const int r = blockIdx.x;
    if (r >= I.rows) return;
    const unsigned char* m = I.mask + (size_t)r * I.cols;
    int64_t n = 0;
    for (int c0 = 0; c0 < I.cols; c0 += 64) {
        const int c = c0 + threadIdx.x;
        n += __popcll(__ballot(c < I.cols && m[c] != 0));
    }
    if (threadIdx.x == 0) rowcnt[I.row_base + r] = n;
}

__global__ void cmp_scan_kernel(CmpItem* __restrict__ items, int n_items, int64_t* __restrict__ rowcnt)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_items) return;
    CmpItem& I = items[k];
    int64_t run = 0;
    for (int r = 0; r < I.rows; ++r) {
        const int64_t c = rowcnt[I.row_base + r];
        rowcnt[I.row_base + r] = run;
        run += c;
    }
    I.n = run;
}

__global__ void __launch_bounds__(64) cmp_write_kernel(const CmpItem* __restrict__ items, const int64_t* __restrict__ rowoff)
{
    const CmpItem& I = items[blockIdx.y];
    const int r = blockIdx.x;
    if (r >= I.rows || !I.out) return;
    const unsigned char* m = I.mask + (size_t)r * I.cols;
    int64_t at = rowoff[I.row_base + r];
    const unsigned long long lt = (1ull << threadIdx.x) - 1ull;
    for (int c0 = 0; c0 < I.cols; c0 += 64) {
        const int c = c0 + threadIdx.x;
        const bool on = c < I.cols && m[c] != 0;
        const unsigned long long b = __ballot(on);
        if (on) {
            const float* s = I.pts + ((size_t)r * I.cols + c) * 6;
            float* d = I.out + (size_t)(at + __popcll(b & lt)) * 6;
            for (int q = 0; q < 6; ++q) d[q] = s[q];
        }
        at += __popcll(b);
    }
}

// Centroid of an item's xyz: thread k sums points k, k + 256, ... in float64, a fixed tree combines them (0 points: NaN, like np.mean).
constexpr int CENT_THREADS = 256;
__global__ void __launch_bounds__(CENT_THREADS) centroid_kernel(const CmpItem* __restrict__ items, double* __restrict__ cent)
{
    __shared__ double s[3][CENT_THREADS];
    const CmpItem& I = items[blockIdx.x];
    double a[3] = {0.0, 0.0, 0.0};
    for (int64_t p = threadIdx.x; p < I.n; p += CENT_THREADS)
        for (int q = 0; q < 3; ++q) a[q] += (double)I.out[(size_t)p * 6 + q];
    for (int q = 0; q < 3; ++q) s[q][threadIdx.x] = a[q];
    __syncthreads();
    for (int w = CENT_THREADS / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w)
            for (int q = 0; q < 3; ++q) s[q][threadIdx.x] += s[q][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 3) cent[3 * blockIdx.x + threadIdx.x] = s[threadIdx.x][0] / (double)I.n;
}

// points_src[:, :3] += centroid_tgt - centroid_src (float32 array, float64 operand: the sum is formed in float64, stored as float32)
__global__ void __launch_bounds__(256) shift_kernel(const CmpItem* __restrict__ items, const int* __restrict__ job_of,
                                                    const double* __restrict__ ctgt, const double* __restrict__ csrc)
{
    const CmpItem& I = items[blockIdx.y];
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= I.n || !I.out) return;
    const int j = job_of[blockIdx.y];
    for (int q = 0; q < 3; ++q) {
        const double adj = ctgt[3 * j + q] - csrc[3 * blockIdx.y + q];
        float* x = I.out + (size_t)p * 6 + q;
        *x = (float)((double)*x + adj);
    }
}

// Init_mask statistics of a job over the whole frame: bounding box (get_bbox_from_mask, inclusive max) and pixel count.
constexpr int BOX_THREADS = 256;
__global__ void __launch_bounds__(BOX_THREADS) init_box_kernel(const float* __restrict__ zbuf, const unsigned char* __restrict__ umask,
                                                               int H, int W, int* __restrict__ box)
{
    __shared__ int s[5][BOX_THREADS];
    const size_t HW = (size_t)H * W;
    const float* z = zbuf + blockIdx.x * HW;
    const unsigned char* m = umask + blockIdx.x * HW;
    int rmin = H, cmin = W, rmax = -1, cmax = -1, n = 0;
    for (size_t p = threadIdx.x; p < HW; p += BOX_THREADS)
        if (z[p] > 0.0f && m[p]) {
            const int r = (int)(p / W), c = (int)(p % W);
            rmin = min(rmin, r); rmax = max(rmax, r); cmin = min(cmin, c); cmax = max(cmax, c); ++n;
        }
    s[0][threadIdx.x] = rmin; s[1][threadIdx.x] = cmin; s[2][threadIdx.x] = rmax; s[3][threadIdx.x] = cmax; s[4][threadIdx.x] = n;
    __syncthreads();
    for (int w = BOX_THREADS / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            const int o = threadIdx.x + w;
            s[0][threadIdx.x] = min(s[0][threadIdx.x], s[0][o]);
            s[1][threadIdx.x] = min(s[1][threadIdx.x], s[1][o]);
            s[2][threadIdx.x] = max(s[2][threadIdx.x], s[2][o]);
            s[3][threadIdx.x] = max(s[3][threadIdx.x], s[3][o]);
            s[4][threadIdx.x] += s[4][o];
        }
        __syncthreads();
    }
    if (threadIdx.x < 5) box[5 * blockIdx.x + threadIdx.x] = s[threadIdx.x][0];
}

// The normalised float64 weights of ndimage.gaussian_filter(., 2) (scipy _gaussian_kernel1d: exp(-0.5 / sigma^2 x^2) / sum), centre
// first; summed in the order x = -8 .. 8.
GaussW gauss_weights()
{
    double phi[2 * GAUSS_R + 1], sum = 0.0;
    for (int x = -GAUSS_R; x <= GAUSS_R; ++x) phi[x + GAUSS_R] = std::exp(-0.5 / 4.0 * (double)(x * x));
    for (int k = 0; k < 2 * GAUSS_R + 1; ++k) sum += phi[k];
    GaussW g;
    for (int k = 0; k <= GAUSS_R; ++k) g.w[k] = phi[GAUSS_R + k] / sum;
    return g;
}

// Fill, Gaussian and normals of n items already in device memory (ditems; host copy `items` gives the launch extents).
int run_items(hipStream_t st, const std::vector<NrmItem>& items, const NrmItem* ditems, int H, int W)
{
    if (items.empty()) return P2P_OK;
    int mrh = 1, mrw = 1, mgh = 1, mgw = 1;
    for (const NrmItem& I : items) {
        mrh = std::max(mrh, I.rh); mrw = std::max(mrw, I.rw); mgh = std::max(mgh, I.gh); mgw = std::max(mgw, I.gw);
    }
    const unsigned n = (unsigned)items.size();
    const dim3 blk(TX, TY), gr((mrw + TX - 1) / TX, (mrh + TY - 1) / TY, n), gc((mgw + TX - 1) / TX, (mgh + TY - 1) / TY, n);
    fill_init_kernel<<<gr, blk, 0, st>>>(ditems, W);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < FILL_LAYERS; ++k) {
        fill_layer_kernel<<<gr, blk, 0, st>>>(ditems, k & 1);
        HIP_TRY(hipGetLastError());
    }
    const GaussW g = gauss_weights();
    gauss_kernel<0><<<gr, blk, 0, st>>>(ditems, H, W, g, FILL_LAYERS & 1);
    HIP_TRY(hipGetLastError());
    gauss_kernel<1><<<gr, blk, 0, st>>>(ditems, H, W, g, FILL_LAYERS & 1);
    HIP_TRY(hipGetLastError());
    normal_kernel<<<gc, blk, 0, st>>>(ditems, W);
    HIP_TRY(hipGetLastError());
    return P2P_OK;
}

// Per-item work buffers of `items` (regions and crops set): carves fa/fb/tmp/sm (and pts/cmask where null) out of one allocation.
int alloc_items(std::vector<NrmItem>& items, DevBuf& buf, bool want_pts)
{
    size_t total = 0;
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    for (const NrmItem& I : items) {
        const size_t rn = (size_t)I.rh * I.rw, gn = (size_t)I.gh * I.gw;
        total += 2 * up(rn * 4) + 2 * up(rn * 8) + (want_pts ? up(gn * 24) + up(gn) : 0);
    }
    int rc;
    if ((rc = buf.reserve(std::max<size_t>(total, 256)))) return rc;
    char* p = buf.as<char>();
    for (NrmItem& I : items) {
        const size_t rn = (size_t)I.rh * I.rw, gn = (size_t)I.gh * I.gw;
        I.fa = reinterpret_cast<float*>(p); p += up(rn * 4);
        I.fb = reinterpret_cast<float*>(p); p += up(rn * 4);
        I.tmp = reinterpret_cast<double*>(p); p += up(rn * 8);
        I.sm = reinterpret_cast<double*>(p); p += up(rn * 8);
        if (want_pts) {
            I.pts = reinterpret_cast<float*>(p); p += up(gn * 24);
            I.cmask = reinterpret_cast<unsigned char*>(p); p += up(gn);
        }
    }
    return P2P_OK;
}

int check_size(const char* who, int H, int W)
{
    if (H < 3 || W < 3 || H > MAX_SIDE || W > MAX_SIDE || (int64_t)H * W > (1 << 26)) {
        set_error("%s: image size %d x %d (np.gradient needs 3 samples per axis; at most %d per side, 2^26 pixels)", who, H, W, MAX_SIDE);
        return P2P_ERR_INVALID_ARG;
    }
    return P2P_OK;
}

int check_cam(const char* who, const double* K, int idx)
{
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    if (!std::isfinite(fx) || !std::isfinite(fy) || fx == 0.0 || fy == 0.0 || !(std::fabs(cx) < MAX_SIDE) || !(std::fabs(cy) < MAX_SIDE)) {
        set_error("%s: camera %d: fx %g fy %g cx %g cy %g (finite, fx, fy nonzero, |cx|, |cy| < %d)", who, idx, fx, fy, cx, cy, MAX_SIDE);
        return P2P_ERR_INVALID_ARG;
    }
    return P2P_OK;
}

NrmItem frame_item(const float* depth, const double* K, int H, int W)
{
    NrmItem I{};
    I.depth = depth;
    I.r0 = 0; I.c0 = 0; I.rh = H; I.rw = W;
    I.g0 = 0; I.gc0 = 0; I.gh = H; I.gw = W;
    I.fx = K[0]; I.fy = K[4]; I.cx = K[2]; I.cy = K[5];
    return I;
}

// Scene points of n frames: uploads depth_images[img[f]] and runs fill, Gaussian and normals with camera cams[f] into dpts
// [n][H][W][6] (asynchronous).
int frame_points(hipStream_t st, const float* const* depth_images, const int* img, const double* const* cams, int n, int H, int W,
                 DevBuf& dimg, DevBuf& dpts, DevBuf& dwork, DevBuf& ditems, bool dev_inputs = false)
{
    const size_t HW = (size_t)H * W;
    int rc;
    if ((rc = dimg.reserve(n * HW * 4)) || (rc = dpts.reserve(n * HW * 24))) return rc;
    std::vector<NrmItem> items(n);
    for (int f = 0; f < n; ++f) {
        items[f] = frame_item(dimg.as<float>() + f * HW, cams[f], H, W);
        items[f].pts = dpts.as<float>() + f * HW * 6;
    }
    if ((rc = alloc_items(items, dwork, false)) || (rc = ditems.reserve(sizeof(NrmItem) * n))) return rc;
    for (int f = 0; f < n; ++f)
        HIP_TRY(hipMemcpyAsync(dimg.as<float>() + f * HW, depth_images[img[f]], HW * 4,
                               dev_inputs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ditems.p, items.data(), sizeof(NrmItem) * n, hipMemcpyHostToDevice, st));
    return run_items(st, items, ditems.as<NrmItem>(), H, W);
}

// Compaction, step 1: count and scan the rows of `items`; on return items[k].n holds the item's point count (synchronises).
int compact_count(hipStream_t st, std::vector<CmpItem>& items, DevBuf& ditems, DevBuf& drow)
{
    const int n = (int)items.size();
    int64_t rows = 0;
    int max_rows = 1;
    for (CmpItem& I : items) { I.row_base = rows; rows += I.rows; max_rows = std::max(max_rows, I.rows); }
    int rc;
    if ((rc = ditems.reserve(sizeof(CmpItem) * n)) || (rc = drow.reserve(sizeof(int64_t) * std::max<int64_t>(rows, 1)))) return rc;
    HIP_TRY(hipMemcpyAsync(ditems.p, items.data(), sizeof(CmpItem) * n, hipMemcpyHostToDevice, st));
    cmp_count_kernel<<<dim3(max_rows, n), 64, 0, st>>>(ditems.as<CmpItem>(), drow.as<int64_t>());
    HIP_TRY(hipGetLastError());
    cmp_scan_kernel<<<(n + 63) / 64, 64, 0, st>>>(ditems.as<CmpItem>(), n, drow.as<int64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(items.data(), ditems.p, sizeof(CmpItem) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return P2P_OK;
}

// Compaction, step 2: with the out pointers set, write every item's points at the row offsets step 1 left in drow.
int compact_write(hipStream_t st, const std::vector<CmpItem>& items, DevBuf& ditems, const DevBuf& drow)
{
    int max_rows = 1;
    for (const CmpItem& I : items) max_rows = std::max(max_rows, I.rows);
    HIP_TRY(hipMemcpyAsync(ditems.p, items.data(), sizeof(CmpItem) * items.size(), hipMemcpyHostToDevice, st));
    cmp_write_kernel<<<dim3(max_rows, (unsigned)items.size()), 64, 0, st>>>(ditems.as<CmpItem>(), drow.as<int64_t>());
    HIP_TRY(hipGetLastError());
    return P2P_OK;
}

}  // namespace
}  // namespace p2p

using namespace p2p;

extern "C" {

int p2p_depth_points_batch(p2p_ctx* ctx, const float* const* depth_images, int n_images, const double* camK, int height, int width,
                           float* points)
{
    const char* who = "p2p_depth_points_batch";
    if (!ctx || n_images < 0 || n_images > 65535 || (n_images > 0 && (!depth_images || !camK || !points))) {
        set_error("%s: bad arguments", who);
        return P2P_ERR_INVALID_ARG;
    }
    int rc;
    if ((rc = check_size(who, height, width))) return rc;
    for (int i = 0; i < n_images; ++i) {
        if (!depth_images[i]) {
            set_error("%s: depth image %d is null", who, i);
            return P2P_ERR_INVALID_ARG;
        }
        if ((rc = check_cam(who, camK + 9 * i, i))) return rc;
    }
    if (n_images == 0) return P2P_OK;
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t HW = (size_t)height * width;
    DevBuf dimg, dpts, dwork, ditems;
    std::vector<int> img(n_images);
    std::vector<const double*> cams(n_images);
    for (int i = 0; i < n_images; ++i) { img[i] = i; cams[i] = camK + 9 * i; }
    if ((rc = frame_points(st, depth_images, img.data(), cams.data(), n_images, height, width, dimg, dpts, dwork, ditems))) return rc;
    HIP_TRY(hipMemcpyAsync(points, dpts.p, n_images * HW * 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return P2P_OK;
}

}  // extern "C"

namespace p2p {

int icp_inputs_stage(const char* who, p2p_ctx* ctx, const p2p_mesh* const* meshes, int n_meshes, const float* const* depth_images,
                     int n_images, const p2p_refine_job* jobs, int n_jobs, int height, int width, p2p_icp_input* out, IcpInputsStage& S,
                     bool dev_inputs)
{
    if (!ctx || n_jobs < 0 || n_jobs > 65535 || n_images < 0 || (n_jobs > 0 && (!meshes || !jobs || !out || !depth_images))) {
        set_error("%s: bad arguments", who);
        return P2P_ERR_INVALID_ARG;
    }
    int rc;
    if ((rc = check_size(who, height, width))) return rc;
    if ((rc = check_jobs(who, meshes, n_meshes, jobs, n_jobs, height, width, n_images))) return rc;
    for (int j = 0; j < n_jobs; ++j)
        if ((rc = check_cam(who, jobs[j].camK, j))) return rc;
    for (int j = 0; j < n_jobs; ++j)
        if (!depth_images[jobs[j].img_idx]) {
            set_error("%s: depth image %d is null", who, jobs[j].img_idx);
            return P2P_ERR_INVALID_ARG;
        }
    if (n_jobs == 0) return P2P_OK;
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t HW = (size_t)height * width;
    const bool whole = dev_env("P2P_NORMALS_WHOLE") != nullptr;     // development twin: jobs' fill and Gaussian over the whole frame

    // the buffers are S's and live until the caller's stage goes out of scope; each has one use (DevBuf::reserve frees before it grows,
    // so a buffer read by queued work is never reserved again)
    // 1. the sensor frames the jobs name and the union masks; scene points of each frame once per camera it is seen with (the reference
    //    computes points_tgt once per image with that image's cam_K, icp3d.py:372-374)
    std::vector<int> frames, frame_job, slot_of(n_jobs);      // frame -> image, first job naming it; job -> frame
    for (int j = 0; j < n_jobs; ++j) {
        int f = 0;
        while (f < (int)frames.size() &&
               !(frames[f] == jobs[j].img_idx && std::memcmp(jobs[frame_job[f]].camK, jobs[j].camK, sizeof(jobs[j].camK)) == 0))
            ++f;
        if (f == (int)frames.size()) {
            frames.push_back(jobs[j].img_idx);
            frame_job.push_back(j);
        }
        slot_of[j] = f;
    }
    const int nf = (int)frames.size();
    std::vector<const double*> cams(nf);
    for (int f = 0; f < nf; ++f) cams[f] = jobs[frame_job[f]].camK;
    if ((rc = frame_points(st, depth_images, frames.data(), cams.data(), nf, height, width, S.dimg, S.dscene, S.dwork, S.ditems,
                           dev_inputs)))
        return rc;
    if ((rc = S.dumask.reserve(n_jobs * HW))) return rc;
    for (int j = 0; j < n_jobs; ++j)
        HIP_TRY(hipMemcpyAsync(S.dumask.as<unsigned char>() + j * HW, jobs[j].union_mask, HW,
                               dev_inputs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));

    // 2. target points pts_tgt = points_tgt[union_mask] (:464) and their centroid (icp_refinement :59)
    std::vector<CmpItem> titems(n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        CmpItem& T = titems[j];
        T = CmpItem{};
        T.pts = S.dscene.as<float>() + slot_of[j] * HW * 6;
        T.mask = S.dumask.as<unsigned char>() + j * HW;
        T.rows = height; T.cols = width;
    }
    if ((rc = compact_count(st, titems, S.dcmp, S.drow))) return rc;
    int64_t tot_tgt = 0;
    std::vector<int64_t> tgt_off(n_jobs);
    for (int j = 0; j < n_jobs; ++j) { tgt_off[j] = tot_tgt; tot_tgt += titems[j].n; }
    if ((rc = S.dtgt.reserve(std::max<int64_t>(tot_tgt, 1) * 24))) return rc;
    for (int j = 0; j < n_jobs; ++j) titems[j].out = S.dtgt.as<float>() + tgt_off[j] * 6;
    if ((rc = compact_write(st, titems, S.dcmp, S.drow))) return rc;
    if ((rc = S.dctgt.reserve(sizeof(double) * 3 * n_jobs))) return rc;
    centroid_kernel<<<n_jobs, CENT_THREADS, 0, st>>>(S.dcmp.as<CmpItem>(), S.dctgt.as<double>());
    HIP_TRY(hipGetLastError());
    std::vector<double> ctgt(3 * n_jobs);
    HIP_TRY(hipMemcpyAsync(ctgt.data(), S.dctgt.p, sizeof(double) * 3 * n_jobs, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));

    // 3. t replacement (:60-61) and the render at that pose (:64-67)
    std::vector<p2p_refine_job> rj(jobs, jobs + n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        p2p_icp_input& R = out[j];
        std::memset(&R, 0, sizeof(R));
        R.n_tgt = titems[j].n;
        R.tgt_offset = tgt_off[j];
        for (int q = 0; q < 3; ++q) R.centroid_tgt[q] = ctgt[3 * j + q];
        const bool replace = jobs[j].t[2] < 300.0 || jobs[j].t[2] > 5000.0;
        for (int q = 0; q < 3; ++q) R.t_init[q] = rj[j].t[q] = replace ? ctgt[3 * j + q] * 1000.0 : jobs[j].t[q];
    }
    if ((rc = S.dz.reserve(n_jobs * HW * 4))) return rc;
    if ((rc = render_into(*c, meshes, rj.data(), n_jobs, height, width, S.dz.as<unsigned>(), S.dj))) return rc;

    // 4. init_mask, its bbox and the two gates (:68-74)
    if ((rc = S.dbox.reserve(sizeof(int) * 5 * n_jobs))) return rc;
    init_box_kernel<<<n_jobs, BOX_THREADS, 0, st>>>(S.dz.as<float>(), S.dumask.as<unsigned char>(), height, width, S.dbox.as<int>());
    HIP_TRY(hipGetLastError());
    std::vector<int> box(5 * n_jobs);
    HIP_TRY(hipMemcpyAsync(box.data(), S.dbox.p, sizeof(int) * 5 * n_jobs, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<NrmItem> sitems;
    std::vector<int> job_of;
    for (int j = 0; j < n_jobs; ++j) {
        p2p_icp_input& R = out[j];
        const int* b = &box[5 * j];
        if (b[4] > 0)
            for (int q = 0; q < 4; ++q) R.bbox[q] = b[q];
        if (R.bbox[2] - R.bbox[0] < 5 || R.bbox[3] - R.bbox[1] < 5)
            R.status = P2P_ICP_SMALL_BBOX;
        else if (b[4] < 10)
            R.status = P2P_ICP_FEW_POINTS;
        if (R.status != P2P_ICP_OK) continue;
        // points_src over [rmin, rmax) x [cmin, cmax): the inclusive max of get_bbox_from_mask used as an exclusive slice end
        NrmItem I = frame_item(S.dz.as<float>() + j * HW, jobs[j].camK, height, width);
        I.umask = S.dumask.as<unsigned char>() + j * HW;
        I.g0 = R.bbox[0]; I.gc0 = R.bbox[1]; I.gh = R.bbox[2] - R.bbox[0]; I.gw = R.bbox[3] - R.bbox[1];
        if (!whole) {
            I.r0 = std::max(0, I.g0 - NRM_GROW); I.c0 = std::max(0, I.gc0 - NRM_GROW);
            I.rh = std::min(height, I.g0 + I.gh + NRM_GROW) - I.r0; I.rw = std::min(width, I.gc0 + I.gw + NRM_GROW) - I.c0;
        }
        sitems.push_back(I);
        job_of.push_back(j);
    }

    // 5. source points with normals over the crop (:75-78), compacted in row-major order, their centroid and the shift (:80-84)
    const int ns = (int)sitems.size();
    std::vector<CmpItem> citems(ns);
    if (ns > 0) {
        if ((rc = alloc_items(sitems, S.dwork2, true))) return rc;
        if ((rc = S.ditems2.reserve(sizeof(NrmItem) * ns))) return rc;
        HIP_TRY(hipMemcpyAsync(S.ditems2.p, sitems.data(), sizeof(NrmItem) * ns, hipMemcpyHostToDevice, st));
        if ((rc = run_items(st, sitems, S.ditems2.as<NrmItem>(), height, width))) return rc;
        for (int k = 0; k < ns; ++k) {
            citems[k] = CmpItem{};
            citems[k].pts = sitems[k].pts;
            citems[k].mask = sitems[k].cmask;
            citems[k].rows = sitems[k].gh; citems[k].cols = sitems[k].gw;
        }
        if ((rc = compact_count(st, citems, S.dcmp2, S.drow2))) return rc;
    }
    int64_t tot_src = 0;
    for (int j = 0, k = 0; j < n_jobs; ++j) {      // packed in job order; a gated job has no source points and keeps t = t_init
        out[j].src_offset = tot_src;
        if (k < ns && job_of[k] == j) {
            out[j].n_src = citems[k].n;
            tot_src += citems[k++].n;
        } else {
            for (int q = 0; q < 3; ++q) out[j].t_adjusted[q] = out[j].t_init[q];
        }
    }
    if (ns > 0) {
        if ((rc = S.dsrc.reserve(std::max<int64_t>(tot_src, 1) * 24))) return rc;
        for (int k = 0; k < ns; ++k) citems[k].out = S.dsrc.as<float>() + out[job_of[k]].src_offset * 6;
        if ((rc = compact_write(st, citems, S.dcmp2, S.drow2))) return rc;
        if ((rc = S.dcsrc.reserve(sizeof(double) * 3 * ns))) return rc;
        if ((rc = S.djob_of.reserve(sizeof(int) * ns))) return rc;
        HIP_TRY(hipMemcpyAsync(S.djob_of.p, job_of.data(), sizeof(int) * ns, hipMemcpyHostToDevice, st));
        centroid_kernel<<<ns, CENT_THREADS, 0, st>>>(S.dcmp2.as<CmpItem>(), S.dcsrc.as<double>());
        HIP_TRY(hipGetLastError());
        int64_t maxn = 1;
        for (int k = 0; k < ns; ++k) maxn = std::max(maxn, citems[k].n);
        shift_kernel<<<dim3((unsigned)((maxn + 255) / 256), ns), 256, 0, st>>>(S.dcmp2.as<CmpItem>(), S.djob_of.as<int>(),
                                                                             S.dctgt.as<double>(), S.dcsrc.as<double>());
        HIP_TRY(hipGetLastError());
        std::vector<double> csrc(3 * ns);
        HIP_TRY(hipMemcpyAsync(csrc.data(), S.dcsrc.p, sizeof(double) * 3 * ns, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int k = 0; k < ns; ++k) {
            p2p_icp_input& R = out[job_of[k]];
            for (int q = 0; q < 3; ++q) {
                R.centroid_src[q] = csrc[3 * k + q];
                R.t_adjusted[q] = R.t_init[q] + (R.centroid_tgt[q] - R.centroid_src[q]) * 1000.0;
            }
        }
    }

    S.slot_of = slot_of;
    S.tot_src = tot_src;
    S.tot_tgt = tot_tgt;
    return P2P_OK;
}

}  // namespace p2p

extern "C" {

int p2p_icp_inputs_batch(p2p_ctx* ctx, const p2p_mesh* const* meshes, int n_meshes, const float* const* depth_images, int n_images,
                         const p2p_refine_job* jobs, int n_jobs, int height, int width, p2p_icp_input* out, float* src_points,
                         int64_t src_capacity, float* tgt_points, int64_t tgt_capacity)
{
    const char* who = "p2p_icp_inputs_batch";
    if (src_capacity < 0 || tgt_capacity < 0) {
        set_error("%s: bad arguments", who);
        return P2P_ERR_INVALID_ARG;
    }
    IcpInputsStage S;
    int rc = icp_inputs_stage(who, ctx, meshes, n_meshes, depth_images, n_images, jobs, n_jobs, height, width, out, S);
    if (rc || n_jobs == 0) return rc;
    hipStream_t st = reinterpret_cast<Ctx*>(ctx)->stream;

    // the point buffers, if they are given and large enough
    if ((src_points && S.tot_src > src_capacity) || (tgt_points && S.tot_tgt > tgt_capacity)) {
        set_error("%s: %lld source / %lld target points, capacities %lld / %lld", who, (long long)S.tot_src, (long long)S.tot_tgt,
                  (long long)src_capacity, (long long)tgt_capacity);
        return P2P_ERR_CAPACITY;
    }
    if (src_points && S.tot_src > 0) HIP_TRY(hipMemcpyAsync(src_points, S.dsrc.p, S.tot_src * 24, hipMemcpyDeviceToHost, st));
    if (tgt_points && S.tot_tgt > 0) HIP_TRY(hipMemcpyAsync(tgt_points, S.dtgt.p, S.tot_tgt * 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return P2P_OK;
}

}  // extern "C"
