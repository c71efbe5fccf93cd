// Training patches from XYZ colour renders (reference tools/2_2_render_pix2pose_training.py:168-184): crop [rgb | xyz] to the render's
// box, grey where nothing is drawn, the 8-bit colour read-back rule, and for boxes above 128 px the skimage resize of each half with
// the sampling rules the est_pose resizes use (resize_rules.h).  DESIGN.md section 8.4; tests/xyz_ref.py restates it.
#include <hip/hip_runtime.h>

#include <vector>

#include "model.h"
#include "pipeline.h"
#include "resize_rules.h"

#pragma clang fp contract(off)

namespace p2p {

namespace {

constexpr int PATCH = 128;

struct PatchJob {
    int r0, c0, h, w;      // crop: rows r0 .. r0 + h, columns c0 .. c0 + w of the frame (h = 0: skipped job)
    int oh, ow;            // stored shape
    // generations 1 and 2, resized jobs: the two halves [h][w][3] as float32(x / 255) held in doubles -- cv as built, src after the
    // Gaussian pre-filter (whichever buffer the last pass of non-zero radius wrote)
    double* cv[2];
    const double* src[2];
};

// The uint8 the reference's patch holds for colour c: the GL buffer's level q = floor(c * 255 + 0.5), read back as float32(q) / 255,
// multiplied by 255 in float32 and truncated (for some q this is q - 1).
__device__ __forceinline__ unsigned char xyz_level(float c)
{
    const double q = floor((double)c * 255.0 + 0.5);
    const float back = (float)q / 255.0f;
    return (unsigned char)(back * 255.0f);
}

// channel ch (0..2 rgb, 3..5 xyz) of the unresized patch at frame pixel (y, x)
__device__ __forceinline__ unsigned char patch_src(const unsigned char* __restrict__ rgb, const float* __restrict__ color,
                                                   const float* __restrict__ depth, int W, int y, int x, int ch)
{
    const size_t p = (size_t)y * W + x;
    if (ch < 3) return depth[p] == 0.f ? (unsigned char)128 : rgb[p * 3 + ch];
    return xyz_level(color[p * 3 + (ch - 3)]);
}

// [min, max] of each half of the crop as uint8 (x -> float32(x / 255) is monotone): what skimage's clip=True clamps the warp to.
// range [n][4] = min rgb, max rgb, min xyz, max xyz; starts at 255, 0, 255, 0.  Only jobs that are resized need it.
__global__ void __launch_bounds__(256) patch_range_kernel(const PatchJob* __restrict__ jobs, const unsigned char* __restrict__ rgb,
                                                          const float* __restrict__ color, const float* __restrict__ depth, int H,
                                                          int W, int* __restrict__ range)
{
    const PatchJob J = jobs[blockIdx.y];
    if (J.h == 0 || (J.oh == J.h && J.ow == J.w)) return;
    const size_t HW = (size_t)H * W;
    const unsigned char* f = rgb + blockIdx.y * HW * 3;
    const float* c = color + blockIdx.y * HW * 3;
    const float* d = depth + blockIdx.y * HW;
    int lo[2] = {255, 255}, hi[2] = {0, 0};
    const int n = J.h * J.w;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const int y = J.r0 + e / J.w, x = J.c0 + e % J.w;
        for (int ch = 0; ch < 6; ++ch) {
            const int v = patch_src(f, c, d, W, y, x, ch);
            lo[ch / 3] = min(lo[ch / 3], v); hi[ch / 3] = max(hi[ch / 3], v);
        }
    }
    for (int o = 32; o > 0; o >>= 1)
        for (int k = 0; k < 2; ++k) { lo[k] = min(lo[k], __shfl_down(lo[k], o, 64)); hi[k] = max(hi[k], __shfl_down(hi[k], o, 64)); }
    if ((threadIdx.x & 63) == 0 && lo[0] <= hi[0]) {
        int* r = range + 4 * blockIdx.y;
        atomicMin(r + 0, lo[0]); atomicMax(r + 1, hi[0]); atomicMin(r + 2, lo[1]); atomicMax(r + 3, hi[1]);
    }
}

// Generations 1 and 2: the halves of a resized job as images for the pre-filter.
__global__ void __launch_bounds__(256) patch_canvas_kernel(const PatchJob* __restrict__ jobs, const unsigned char* __restrict__ rgb,
                                                           const float* __restrict__ color, const float* __restrict__ depth, int H, int W)
{
    const PatchJob J = jobs[blockIdx.y];
    if (J.h == 0 || !J.cv[0]) return;
    const size_t HW = (size_t)H * W;
    const unsigned char* f = rgb + blockIdx.y * HW * 3;
    const float* c = color + blockIdx.y * HW * 3;
    const float* d = depth + blockIdx.y * HW;
    const int n = J.h * J.w;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const int y = J.r0 + e / J.w, x = J.c0 + e % J.w;
        for (int ch = 0; ch < 6; ++ch)
            J.cv[ch / 3][(size_t)e * 3 + ch % 3] = (double)(float)((double)patch_src(f, c, d, W, y, x, ch) / 255.0);
    }
}

// [min, max] of each filtered half (what clip=True clamps the warp to).  The values are >= 0 (non-negative samples, positive
// weights), so their bit patterns order like the values.  frange [n][4] = min, max of half 0, min, max of half 1 as bits.
__global__ void __launch_bounds__(256) patch_frange_kernel(const PatchJob* __restrict__ jobs, unsigned long long* __restrict__ frange)
{
    const PatchJob J = jobs[blockIdx.y];
    if (J.h == 0 || !J.cv[0]) return;
    const int n = J.h * J.w * 3;
    for (int k = 0; k < 2; ++k) {
        unsigned long long lo = ~0ull, hi = 0ull;
        for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(J.src[k][e]);
            lo = b < lo ? b : lo; hi = b > hi ? b : hi;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long l2 = __shfl_down(lo, o, 64), h2 = __shfl_down(hi, o, 64);
            lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
        }
        if ((threadIdx.x & 63) == 0 && lo <= hi) {
            atomicMin(frange + 4 * blockIdx.y + 2 * k, lo); atomicMax(frange + 4 * blockIdx.y + 2 * k + 1, hi);
        }
    }
}

// One thread per output pixel of the 128 x 128 slot of job blockIdx.y (six bytes).  Unresized: the source bytes.  Resized (generation
// 0: no pre-filter, everything in double): bilinear taps of float32(x / 255) by the shared rules, clipped to the half's range, times 255,
// truncated.
__global__ void __launch_bounds__(256) patch_kernel(const PatchJob* __restrict__ jobs, const unsigned char* __restrict__ rgb,
                                                    const float* __restrict__ color, const float* __restrict__ depth, int H, int W,
                                                    const int* __restrict__ range, const unsigned long long* __restrict__ frange, int gen,
                                                    unsigned char* __restrict__ out)
{
    const PatchJob J = jobs[blockIdx.y];
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int oy = pix / PATCH, ox = pix % PATCH;
    unsigned char o[6] = {0, 0, 0, 0, 0, 0};
    if (oy < J.oh && ox < J.ow) {
        const size_t HW = (size_t)H * W;
        const unsigned char* f = rgb + blockIdx.y * HW * 3;
        const float* c = color + blockIdx.y * HW * 3;
        const float* d = depth + blockIdx.y * HW;
        if (J.oh == J.h && J.ow == J.w) {
            for (int ch = 0; ch < 6; ++ch) o[ch] = patch_src(f, c, d, W, J.r0 + oy, J.c0 + ox, ch);
        } else if (gen == 1) {
            // scikit-image 0.17 / 0.18: the filtered float32 image warped in float32, clipped and multiplied by 255 in float32
            const TapF tr = axis_tap_f32(oy, J.h, J.oh), tc = axis_tap_f32(ox, J.w, J.ow);
            const int r[2] = {reflect_idx(tr.i0, J.h), reflect_idx(tr.i1, J.h)};
            const int cc[2] = {reflect_idx(tc.i0, J.w), reflect_idx(tc.i1, J.w)};
            for (int ch = 0; ch < 6; ++ch) {
                const double* im = J.src[ch / 3];
                float v[2][2];
                for (int a = 0; a < 2; ++a)
                    for (int e = 0; e < 2; ++e) v[a][e] = (float)im[((size_t)r[a] * J.w + cc[e]) * 3 + ch % 3];
                const float lo = (float)__longlong_as_double((long long)frange[4 * blockIdx.y + 2 * (ch / 3)]);
                const float hi = (float)__longlong_as_double((long long)frange[4 * blockIdx.y + 2 * (ch / 3) + 1]);
                float w = lerp2_f32(v[0][0], v[0][1], v[1][0], v[1][1], tr.d, tc.d);
                w = w < lo ? lo : (w > hi ? hi : w);
                o[ch] = (unsigned char)(w * 255.0f);
            }
        } else if (gen == 2) {
            // scikit-image 0.15 / 0.16: the filtered image warped in double
            const Tap tr = axis_tap(oy, J.h, J.oh), tc = axis_tap(ox, J.w, J.ow);
            const int r[2] = {reflect_idx(tr.i0, J.h), reflect_idx(tr.i1, J.h)};
            const int cc[2] = {reflect_idx(tc.i0, J.w), reflect_idx(tc.i1, J.w)};
            for (int ch = 0; ch < 6; ++ch) {
                const double* im = J.src[ch / 3];
                double v[2][2];
                for (int a = 0; a < 2; ++a)
                    for (int e = 0; e < 2; ++e) v[a][e] = im[((size_t)r[a] * J.w + cc[e]) * 3 + ch % 3];
                const double lo = __longlong_as_double((long long)frange[4 * blockIdx.y + 2 * (ch / 3)]);
                const double hi = __longlong_as_double((long long)frange[4 * blockIdx.y + 2 * (ch / 3) + 1]);
                const double w = clip_warp(lerp2(v[0][0], v[0][1], v[1][0], v[1][1], tr.d, tc.d), lo, hi, 0.0);
                o[ch] = (unsigned char)(w * 255.0);
            }
        } else {
            const Tap tr = axis_tap(oy, J.h, J.oh), tc = axis_tap(ox, J.w, J.ow);
            const int r[2] = {J.r0 + reflect_idx(tr.i0, J.h), J.r0 + reflect_idx(tr.i1, J.h)};
            const int cc[2] = {J.c0 + reflect_idx(tc.i0, J.w), J.c0 + reflect_idx(tc.i1, J.w)};
            const int* rg = range + 4 * blockIdx.y;
            for (int ch = 0; ch < 6; ++ch) {
                double v[2][2];
                for (int a = 0; a < 2; ++a)
                    for (int e = 0; e < 2; ++e) v[a][e] = (double)(float)((double)patch_src(f, c, d, W, r[a], cc[e], ch) / 255.0);
                const double lo = (double)(float)((double)rg[2 * (ch / 3)] / 255.0), hi = (double)(float)((double)rg[2 * (ch / 3) + 1] / 255.0);
                const double w = clip_warp(lerp2(v[0][0], v[0][1], v[1][0], v[1][1], tr.d, tc.d), lo, hi, 0.0);
                o[ch] = (unsigned char)(w * 255.0);
            }
        }
    }
    unsigned char* dst = out + ((size_t)blockIdx.y * PATCH * PATCH + pix) * 6;
    for (int ch = 0; ch < 6; ++ch) dst[ch] = o[ch];
}

}  // namespace

}  // namespace p2p

using namespace p2p;

extern "C" int p2p_xyz_patch_batch(p2p_ctx* ctx, const unsigned char* const* rgb, const float* color, const float* depth, const int* bbox,
                                   int n_jobs, int height, int width, int resize_generation, unsigned char* patches, int* shapes)
{
    if (!ctx || n_jobs < 0 || (n_jobs > 0 && (!rgb || !color || !depth || !bbox || !patches || !shapes))) {
        set_error("p2p_xyz_patch_batch: bad arguments (a null context or buffer)");
        return P2P_ERR_INVALID_ARG;
    }
    if (height <= 0 || width <= 0 || (int64_t)height * width > (1 << 26) || n_jobs > 65535) {
        set_error("p2p_xyz_patch_batch: bad image size %d x %d or more than 65535 jobs (%d)", height, width, n_jobs);
        return P2P_ERR_INVALID_ARG;
    }
    if (resize_generation < 0 || resize_generation > 2) {
        set_error("p2p_xyz_patch_batch: resize generation %d, must be 0, 1 or 2", resize_generation);
        return P2P_ERR_INVALID_ARG;
    }
    std::vector<PatchJob> pj(n_jobs);
    for (int k = 0; k < n_jobs; ++k) {
        const int* b = bbox + 4 * k;
        PatchJob& J = pj[k];
        J = PatchJob{};
        shapes[2 * k] = shapes[2 * k + 1] = 0;
        if (!rgb[k]) {
            set_error("p2p_xyz_patch_batch: job %d: null frame", k);
            return P2P_ERR_INVALID_ARG;
        }
        if (b[0] < 0 && b[1] < 0 && b[2] < 0 && b[3] < 0) continue;      // empty render
        if (b[0] < 0 || b[1] < 0 || b[2] < b[0] || b[3] < b[1] || b[2] >= height || b[3] >= width) {
            set_error("p2p_xyz_patch_batch: job %d: box [%d, %d, %d, %d] outside the %d x %d image", k, b[0], b[1], b[2], b[3], height, width);
            return P2P_ERR_INVALID_ARG;
        }
        const int h = b[2] - b[0], w = b[3] - b[1];
        if (h == 0 || w == 0) continue;
        J.r0 = b[0]; J.c0 = b[1]; J.h = h; J.w = w; J.oh = h; J.ow = w;
        const int m = std::max(h, w);
        if (m > PATCH) {
            const double scale = 128.0 / m;
            J.oh = (int)(h * scale + 0.5); J.ow = (int)(w * scale + 0.5);
            if (J.oh == 0 || J.ow == 0) { J = PatchJob{}; continue; }      // a sliver: nothing to store
        }
        shapes[2 * k] = J.oh; shapes[2 * k + 1] = J.ow;
    }
    if (n_jobs == 0) return P2P_OK;
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    HIP_TRY(hipSetDevice(c->device));
    if (!c->pipe) c->pipe = new Pipeline();
    Pipeline::PatchWork& Wk = c->pipe->patch;
    hipStream_t st = c->stream;
    const size_t HW = (size_t)height * width, n = (size_t)n_jobs * HW;
    int rc;
    if ((rc = Wk.rgb.reserve(n * 3)) || (rc = Wk.color.reserve(n * 12)) || (rc = Wk.depth.reserve(n * 4)) ||
        (rc = Wk.jobs.reserve(sizeof(PatchJob) * n_jobs)) || (rc = Wk.range.reserve(sizeof(int) * 4 * n_jobs)) ||
        (rc = Wk.out.reserve((size_t)n_jobs * PATCH * PATCH * 6)))
        return rc;
    // Generations 1 and 2: skimage filters each half before the warp, sigma = (in / out - 1) / 2 per axis.  Two filter items per
    // half: one carries the row axis' radius and weights (first pass, cv -> cv_tmp), one the column axis' (second pass, back).
    std::vector<AaItem> items;          // [rows of every half ..., columns of every half ...]
    std::vector<double> weights;
    std::vector<unsigned long long> frange0((size_t)n_jobs * 4);
    int max_elems = 0;
    if (resize_generation > 0) {
        size_t cv_doubles = 0;
        for (const PatchJob& J : pj)
            if (J.h && (J.oh != J.h || J.ow != J.w)) cv_doubles += (size_t)J.h * J.w * 6;
        if ((rc = Wk.cv.reserve(cv_doubles * 8)) || (rc = Wk.cv_tmp.reserve(cv_doubles * 8)) ||
            (rc = Wk.frange.reserve(sizeof(unsigned long long) * 4 * n_jobs)))
            return rc;
        std::vector<AaItem> rows, cols;
        std::vector<size_t> woff;
        std::vector<double> w;
        size_t off = 0;
        for (PatchJob& J : pj) {
            if (!(J.h && (J.oh != J.h || J.ow != J.w))) continue;
            const int rr = aa_weights_for_axis(J.h, J.oh, w);
            const size_t wr_off = weights.size();
            weights.insert(weights.end(), w.begin(), w.end());
            const int rcol = aa_weights_for_axis(J.w, J.ow, w);
            const size_t wc_off = weights.size();
            weights.insert(weights.end(), w.begin(), w.end());
            for (int k = 0; k < 2; ++k) {
                double* cv = Wk.cv.as<double>() + off;
                double* tmp = Wk.cv_tmp.as<double>() + off;
                off += (size_t)J.h * J.w * 3;
                AaItem I{};
                I.H = J.h; I.W = J.w; I.C = 3; I.mode = 0; I.round32 = 1; I.cval = 0.0;      // a float32 image in every generation: rounded per pass
                I.kmin = ~0ull; I.kmax = 0ull;
                AaItem R = I, Cc = I;
                R.a = cv; R.tmp = tmp; R.radius = rr;
                // the column pass reads what the row pass wrote; with no row pass (radius 0) it reads the canvas itself and writes the scratch
                Cc.tmp = rr > 0 ? tmp : cv; Cc.a = rr > 0 ? cv : tmp; Cc.radius = rcol;
                rows.push_back(R); cols.push_back(Cc);
                woff.push_back(wr_off); woff.push_back(wc_off);
                J.cv[k] = cv;
                J.src[k] = rcol > 0 ? Cc.a : (rr > 0 ? tmp : cv);
                max_elems = std::max(max_elems, J.h * J.w * 3);
            }
        }
        if ((rc = Wk.weights.reserve(std::max<size_t>(1, weights.size()) * 8)) ||
            (rc = Wk.items.reserve(std::max<size_t>(1, rows.size() * 2) * sizeof(AaItem))))
            return rc;
        for (size_t i = 0; i < rows.size(); ++i) {
            rows[i].w = Wk.weights.as<double>() + woff[2 * i];
            cols[i].w = Wk.weights.as<double>() + woff[2 * i + 1];
        }
        items = rows;
        items.insert(items.end(), cols.begin(), cols.end());
        for (int k = 0; k < n_jobs; ++k) { frange0[4 * k] = frange0[4 * k + 2] = ~0ull; frange0[4 * k + 1] = frange0[4 * k + 3] = 0ull; }
    }
    std::vector<int> range0((size_t)n_jobs * 4);
    for (int k = 0; k < n_jobs; ++k) { range0[4 * k] = range0[4 * k + 2] = 255; range0[4 * k + 1] = range0[4 * k + 3] = 0; }
    for (int k = 0; k < n_jobs; ++k) HIP_TRY(hipMemcpyAsync(Wk.rgb.as<unsigned char>() + k * HW * 3, rgb[k], HW * 3, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(Wk.color.p, color, n * 12, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(Wk.depth.p, depth, n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(Wk.jobs.p, pj.data(), sizeof(PatchJob) * n_jobs, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(Wk.range.p, range0.data(), sizeof(int) * 4 * n_jobs, hipMemcpyHostToDevice, st));
    const int n_items = (int)(items.size() / 2);
    if (n_items > 0) {
        HIP_TRY(hipMemcpyAsync(Wk.items.p, items.data(), sizeof(AaItem) * items.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(Wk.weights.p, weights.data(), weights.size() * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(Wk.frange.p, frange0.data(), sizeof(unsigned long long) * frange0.size(), hipMemcpyHostToDevice, st));
        patch_canvas_kernel<<<dim3(64, n_jobs), 256, 0, st>>>(Wk.jobs.as<PatchJob>(), Wk.rgb.as<unsigned char>(), Wk.color.as<float>(),
                                                              Wk.depth.as<float>(), height, width);
        HIP_TRY(hipGetLastError());
        HIP_TRY(launch_aa_filter_axes(Wk.items.as<AaItem>(), Wk.items.as<AaItem>() + n_items, n_items, max_elems, st));
        patch_frange_kernel<<<dim3(64, n_jobs), 256, 0, st>>>(Wk.jobs.as<PatchJob>(), Wk.frange.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
    }
    patch_range_kernel<<<dim3(64, n_jobs), 256, 0, st>>>(Wk.jobs.as<PatchJob>(), Wk.rgb.as<unsigned char>(), Wk.color.as<float>(),
                                                         Wk.depth.as<float>(), height, width, Wk.range.as<int>());
    HIP_TRY(hipGetLastError());
    patch_kernel<<<dim3(PATCH * PATCH / 256, n_jobs), 256, 0, st>>>(Wk.jobs.as<PatchJob>(), Wk.rgb.as<unsigned char>(), Wk.color.as<float>(),
                                                                    Wk.depth.as<float>(), height, width, Wk.range.as<int>(),
                                                                    Wk.frange.as<unsigned long long>(), n_items > 0 ? resize_generation : 0,
                                                                    Wk.out.as<unsigned char>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(patches, Wk.out.p, (size_t)n_jobs * PATCH * PATCH * 6, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return P2P_OK;
}
