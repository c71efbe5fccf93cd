// Training patches from XYZ colour renders (reference tools/2_2_render_pix2pose_training.py:168-184): crop [rgb | xyz] to the render's
// box, grey where nothing is drawn, the 8-bit colour read-back rule, and for boxes above 128 px the skimage resize of each half with
// the sampling rules the est_pose resizes use (resize_rules.h).  DESIGN.md section 8.4; tests/xyz_ref.py restates it.
#include <hip/hip_runtime.h>

#include <cmath>
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
    const unsigned char* crop;      // CropSrc jobs: the unresized patch, u8 [h][w][6] (r0 = c0 = 0)
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

// Where the unresized patch of a job comes from.  FrameSrc: the frame and its render (p2p_xyz_patch_batch).  CropSrc: bytes already
// built per job (p2p_xyz_rotate_patch_batch: the rotated box).  Everything below -- ranges, canvases, filter, warp, slot -- is shared.
struct FrameSrc {
    const unsigned char* rgb; const float* color; const float* depth; int H, W;
    __device__ __forceinline__ unsigned char operator()(const PatchJob&, int job, int y, int x, int ch) const
    {
        const size_t HW = (size_t)H * W;
        return patch_src(rgb + job * HW * 3, color + job * HW * 3, depth + job * HW, W, y, x, ch);
    }
};
struct CropSrc {
    __device__ __forceinline__ unsigned char operator()(const PatchJob& J, int, int y, int x, int ch) const
    {
        return J.crop[((size_t)y * J.w + x) * 6 + ch];
    }
};

// [min, max] of each half of the crop as uint8 (x -> float32(x / 255) is monotone): what skimage's clip=True clamps the warp to.
// range [n][4] = min rgb, max rgb, min xyz, max xyz; starts at 255, 0, 255, 0.  Only jobs that are resized need it.
template <class Src>
__global__ void __launch_bounds__(256) patch_range_kernel(const PatchJob* __restrict__ jobs, const Src src, int* __restrict__ range)
{
    const PatchJob J = jobs[blockIdx.y];
    if (J.h == 0 || (J.oh == J.h && J.ow == J.w)) return;
    int lo[2] = {255, 255}, hi[2] = {0, 0};
    const int n = J.h * J.w;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const int y = J.r0 + e / J.w, x = J.c0 + e % J.w;
        for (int ch = 0; ch < 6; ++ch) {
            const int v = src(J, blockIdx.y, y, x, ch);
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
template <class Src>
__global__ void __launch_bounds__(256) patch_canvas_kernel(const PatchJob* __restrict__ jobs, const Src src)
{
    const PatchJob J = jobs[blockIdx.y];
    if (J.h == 0 || !J.cv[0]) return;
    const int n = J.h * J.w;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const int y = J.r0 + e / J.w, x = J.c0 + e % J.w;
        for (int ch = 0; ch < 6; ++ch)
            J.cv[ch / 3][(size_t)e * 3 + ch % 3] = (double)(float)((double)src(J, blockIdx.y, y, x, ch) / 255.0);
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
template <class Src>
__global__ void __launch_bounds__(256) patch_kernel(const PatchJob* __restrict__ jobs, const Src src, const int* __restrict__ range,
                                                    const unsigned long long* __restrict__ frange, int gen, unsigned char* __restrict__ out)
{
    const PatchJob J = jobs[blockIdx.y];
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int oy = pix / PATCH, ox = pix % PATCH;
    unsigned char o[6] = {0, 0, 0, 0, 0, 0};
    if (oy < J.oh && ox < J.ow) {
        if (J.oh == J.h && J.ow == J.w) {
            for (int ch = 0; ch < 6; ++ch) o[ch] = src(J, blockIdx.y, J.r0 + oy, J.c0 + ox, ch);
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
                    for (int e = 0; e < 2; ++e) v[a][e] = (double)(float)((double)src(J, blockIdx.y, r[a], cc[e], ch) / 255.0);
                const double lo = (double)(float)((double)rg[2 * (ch / 3)] / 255.0), hi = (double)(float)((double)rg[2 * (ch / 3) + 1] / 255.0);
                const double w = clip_warp(lerp2(v[0][0], v[0][1], v[1][0], v[1][1], tr.d, tc.d), lo, hi, 0.0);
                o[ch] = (unsigned char)(w * 255.0);
            }
        }
    }
    unsigned char* dst = out + ((size_t)blockIdx.y * PATCH * PATCH + pix) * 6;
    for (int ch = 0; ch < 6; ++ch) dst[ch] = o[ch];
}

// The shared second half of both builders: pj[k] describes job k's unresized patch (read through src) and its stored shape; the
// 128 x 128 x 6 slots land in patches (host).  Queued on st behind whatever the caller queued to fill src; returns after the stream
// has drained.
template <class Src>
int finish_patches(Pipeline::PatchWork& Wk, hipStream_t st, std::vector<PatchJob>& pj, const Src& src, int resize_generation,
                   unsigned char* patches)
{
    const int n_jobs = (int)pj.size();
    int rc;
    if ((rc = Wk.jobs.reserve(sizeof(PatchJob) * n_jobs)) || (rc = Wk.range.reserve(sizeof(int) * 4 * n_jobs)) ||
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
    HIP_TRY(hipMemcpyAsync(Wk.jobs.p, pj.data(), sizeof(PatchJob) * n_jobs, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(Wk.range.p, range0.data(), sizeof(int) * 4 * n_jobs, hipMemcpyHostToDevice, st));
    const int n_items = (int)(items.size() / 2);
    if (n_items > 0) {
        HIP_TRY(hipMemcpyAsync(Wk.items.p, items.data(), sizeof(AaItem) * items.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(Wk.weights.p, weights.data(), weights.size() * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(Wk.frange.p, frange0.data(), sizeof(unsigned long long) * frange0.size(), hipMemcpyHostToDevice, st));
        patch_canvas_kernel<<<dim3(64, n_jobs), 256, 0, st>>>(Wk.jobs.as<PatchJob>(), src);
        HIP_TRY(hipGetLastError());
        HIP_TRY(launch_aa_filter_axes(Wk.items.as<AaItem>(), Wk.items.as<AaItem>() + n_items, n_items, max_elems, st));
        patch_frange_kernel<<<dim3(64, n_jobs), 256, 0, st>>>(Wk.jobs.as<PatchJob>(), Wk.frange.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
    }
    patch_range_kernel<<<dim3(64, n_jobs), 256, 0, st>>>(Wk.jobs.as<PatchJob>(), src, Wk.range.as<int>());
    HIP_TRY(hipGetLastError());
    patch_kernel<<<dim3(PATCH * PATCH / 256, n_jobs), 256, 0, st>>>(Wk.jobs.as<PatchJob>(), src, Wk.range.as<int>(),
                                                                    Wk.frange.as<unsigned long long>(), n_items > 0 ? resize_generation : 0,
                                                                    Wk.out.as<unsigned char>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(patches, Wk.out.p, (size_t)n_jobs * PATCH * PATCH * 6, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return P2P_OK;
}

// the stored shape of an h x w box (2_2:172-177); false for a sliver that rounds to nothing
bool stored_shape(int h, int w, int& oh, int& ow)
{
    oh = h; ow = w;
    const int m = std::max(h, w);
    if (m > PATCH) {
        const double scale = 128.0 / m;
        oh = (int)(h * scale + 0.5); ow = (int)(w * scale + 0.5);
    }
    return oh > 0 && ow > 0;
}

// ---- in-plane rotation copies (2_2:64-96, augment_inplane_gen with isYCB=False) ----------------------------------------------------
// skimage.transform.rotate(resize=True) of scikit-image 0.17 / 0.18 as tests/xyz_rot_ref.py restates it.  The host forms each
// angle's matrix and output shape with numpy; the kernels do the warps.

struct RotItem {
    double m[6];            // rows 0 and 1 of the map (x, y, 1) of the rotated image -> (column, row) of the frame
    int job;
    int rh, rw;             // shape of the rotated frame
    int r0, c0, h, w;       // the patch: rows r0 .. r0 + h, columns c0 .. c0 + w of the rotated frame (h = 0: none)
    unsigned char* crop;    // u8 [h][w][6]
};

// Per frame pixel an 8-byte record: the 8-bit levels behind the two float32 images the reference rotates -- the frame with 128 where
// depth == 0, the GL buffer's level q of the colour -- then depth > 0, then 0.  rng [job][4]: min / max of rgb_tab[level] and of
// xyz_tab[level] over the frame as float bits (the tables are >= 0, so the bits order like the values); starts at ~0, 0, ~0, 0.
__global__ void __launch_bounds__(256) rot_levels_kernel(const unsigned char* __restrict__ rgb, const float* __restrict__ color,
                                                         const float* __restrict__ depth, int HW, const float* __restrict__ tabs,
                                                         uint2* __restrict__ lv, unsigned* __restrict__ rng)
{
    const int job = blockIdx.y;
    const unsigned char* f = rgb + (size_t)job * HW * 3;
    const float* c = color + (size_t)job * HW * 3;
    const float* d = depth + (size_t)job * HW;
    unsigned lo[2] = {~0u, ~0u}, hi[2] = {0u, 0u};
    for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
        const bool drawn = d[p] != 0.f;
        unsigned l[6];
        for (int k = 0; k < 3; ++k) {
            l[k] = drawn ? f[(size_t)p * 3 + k] : 128u;
            const double q = floor((double)c[(size_t)p * 3 + k] * 255.0 + 0.5);
            l[3 + k] = (unsigned)(q < 0.0 ? 0.0 : (q > 255.0 ? 255.0 : q));
        }
        for (int k = 0; k < 6; ++k) {
            const unsigned b = __float_as_uint(tabs[256 * (k / 3) + l[k]]);
            lo[k / 3] = min(lo[k / 3], b); hi[k / 3] = max(hi[k / 3], b);
        }
        lv[(size_t)job * HW + p] = make_uint2(l[0] | (l[1] << 8) | (l[2] << 16) | (l[3] << 24), l[4] | (l[5] << 8) | ((d[p] > 0.f ? 1u : 0u) << 16));
    }
    for (int o = 32; o > 0; o >>= 1)
        for (int k = 0; k < 2; ++k) { lo[k] = min(lo[k], __shfl_down(lo[k], o, 64)); hi[k] = max(hi[k], __shfl_down(hi[k], o, 64)); }
    if ((threadIdx.x & 63) == 0 && lo[0] <= hi[0]) {
        unsigned* r = rng + 4 * job;
        atomicMin(r + 0, lo[0]); atomicMax(r + 1, hi[0]); atomicMin(r + 2, lo[1]); atomicMax(r + 3, hi[1]);
    }
}

__device__ __forceinline__ bool inside(long r, long c, int H, int W) { return r >= 0 && r < H && c >= 0 && c < W; }

// rotate(depth > 0 as float64): the warp in double per pixel of the rotated frame, and the box of its positive values (2_2:74-75),
// reduced per wave, per workgroup, then with four atomics.  The clip of the library cannot change which values are positive (the
// mask's range is within [0, 1] and cval = 0 is kept where it falls outside), so none is applied; the mask is not stored.
// box [item][4] = min v, min u, max v, max u; starts at INT_MAX, INT_MAX, -1, -1.
__global__ void __launch_bounds__(256) rot_mask_box_kernel(const RotItem* __restrict__ items, const uint2* __restrict__ lv, int H, int W,
                                                           int* __restrict__ box)
{
    __shared__ int s_bb[4][4];
    const RotItem& I = items[blockIdx.y];
    if ((long long)blockIdx.x * 256 >= (long long)I.rh * I.rw) return;
    const int p = blockIdx.x * 256 + threadIdx.x;
    int vlo = 0x7fffffff, ulo = 0x7fffffff, vhi = -1, uhi = -1;
    if (p < I.rh * I.rw) {
        const int oy = p / I.rw, ox = p - oy * I.rw;
        const double x = (double)ox, y = (double)oy;
        const double c = I.m[0] * x + I.m[1] * y + I.m[2];
        const double r = I.m[3] * x + I.m[4] * y + I.m[5];
        const double fr = floor(r), fc = floor(c);
        const long minr = (long)fr, minc = (long)fc, maxr = (long)ceil(r), maxc = (long)ceil(c);
        const double dr = r - fr, dc = c - fc;
        const uint2* m = lv + (size_t)I.job * H * W;
        const double tl = inside(minr, minc, H, W) ? (double)((m[minr * W + minc].y >> 16) & 1u) : 0.0;
        const double tr = inside(minr, maxc, H, W) ? (double)((m[minr * W + maxc].y >> 16) & 1u) : 0.0;
        const double bl = inside(maxr, minc, H, W) ? (double)((m[maxr * W + minc].y >> 16) & 1u) : 0.0;
        const double br = inside(maxr, maxc, H, W) ? (double)((m[maxr * W + maxc].y >> 16) & 1u) : 0.0;
        const double top = (1.0 - dc) * tl + dc * tr;
        const double bottom = (1.0 - dc) * bl + dc * br;
        if ((1.0 - dr) * top + dr * bottom > 0.0) { vlo = vhi = oy; ulo = uhi = ox; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        vlo = min(vlo, __shfl_down(vlo, o, 64)); ulo = min(ulo, __shfl_down(ulo, o, 64));
        vhi = max(vhi, __shfl_down(vhi, o, 64)); uhi = max(uhi, __shfl_down(uhi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        int* b = s_bb[threadIdx.x >> 6];
        b[0] = vlo; b[1] = ulo; b[2] = vhi; b[3] = uhi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) { vlo = min(vlo, s_bb[w][0]); ulo = min(ulo, s_bb[w][1]); vhi = max(vhi, s_bb[w][2]); uhi = max(uhi, s_bb[w][3]); }
        if (vhi >= 0) {
            atomicMin(box + 4 * blockIdx.y + 0, vlo); atomicMin(box + 4 * blockIdx.y + 1, ulo);
            atomicMax(box + 4 * blockIdx.y + 2, vhi); atomicMax(box + 4 * blockIdx.y + 3, uhi);
        }
    }
}

// One thread per pixel of the rotated box: both float32 images warped by the 0.18 float32 rule -- coordinates, floorf / ceilf and the
// fractions in float32; 1 - dc and 1 - dr in double; the left taps multiplied in double, dc * right tap as a float32 product; sums in
// double, one rounding to float32 -- then clipped to the input's range (cval kept where it lies outside it), times 255 in float32 and
// truncated.  The workgroup's 256 x 6 bytes go through LDS and leave as 32-bit words (every crop starts 16-byte aligned).
__global__ void __launch_bounds__(256) rot_patch_kernel(const RotItem* __restrict__ items, const uint2* __restrict__ lv, int H, int W,
                                                        const float* __restrict__ tabs, const unsigned* __restrict__ rng)
{
    __shared__ float s_tab[512];
    __shared__ unsigned s_out[256 * 6 / 4];
    const RotItem& I = items[blockIdx.y];
    const int n = I.h * I.w;
    const int e0 = blockIdx.x * 256;
    if (e0 >= n) return;
    s_tab[threadIdx.x] = tabs[threadIdx.x]; s_tab[256 + threadIdx.x] = tabs[256 + threadIdx.x];
    __syncthreads();
    const int e = e0 + threadIdx.x;
    unsigned char* o = reinterpret_cast<unsigned char*>(s_out) + threadIdx.x * 6;
    if (e < n) {
        const int oy = e / I.w, ox = e - oy * I.w;
        const float x = (float)(I.c0 + ox), y = (float)(I.r0 + oy);
        const float m0 = (float)I.m[0], m1 = (float)I.m[1], m2 = (float)I.m[2], m3 = (float)I.m[3], m4 = (float)I.m[4], m5 = (float)I.m[5];
        const float c = (m0 * x + m1 * y) + m2;
        const float r = (m3 * x + m4 * y) + m5;
        const float fr = floorf(r), fc = floorf(c);
        const long minr = (long)fr, minc = (long)fc, maxr = (long)ceilf(r), maxc = (long)ceilf(c);
        const float dr = r - fr, dc = c - fc;
        const double one_dc = 1.0 - (double)dc, one_dr = 1.0 - (double)dr;
        const uint2* m = lv + (size_t)I.job * H * W;
        // an outside tap: level record of cval -- 0.5 for the frame, 0 for the colour -- marked in bit 31 of .y
        const uint2 OUT = make_uint2(0u, 0x80000000u);
        const uint2 t[4] = {inside(minr, minc, H, W) ? m[minr * W + minc] : OUT, inside(minr, maxc, H, W) ? m[minr * W + maxc] : OUT,
                            inside(maxr, minc, H, W) ? m[maxr * W + minc] : OUT, inside(maxr, maxc, H, W) ? m[maxr * W + maxc] : OUT};
        const unsigned* g = rng + 4 * I.job;
        for (int ch = 0; ch < 6; ++ch) {
            const float cval = ch < 3 ? 0.5f : 0.f;
            float v[4];
            for (int a = 0; a < 4; ++a) {
                const unsigned l = ch < 4 ? (t[a].x >> (8 * ch)) & 255u : (t[a].y >> (8 * (ch - 4))) & 255u;
                v[a] = (t[a].y >> 31) ? cval : s_tab[256 * (ch / 3) + l];
            }
            const double top = one_dc * (double)v[0] + (double)(dc * v[1]);
            const double bottom = one_dc * (double)v[2] + (double)(dc * v[3]);
            const float wv = (float)(one_dr * top + (double)dr * bottom);
            const float lo = __uint_as_float(g[2 * (ch / 3)]), hi = __uint_as_float(g[2 * (ch / 3) + 1]);
            const bool keep = wv == cval && !(lo <= cval && cval <= hi);
            const float cl = keep ? cval : (wv < lo ? lo : (wv > hi ? hi : wv));
            o[ch] = (unsigned char)(cl * 255.0f);
        }
    } else {
        for (int ch = 0; ch < 6; ++ch) o[ch] = 0;
    }
    __syncthreads();
    const int n_here = min(256, n - e0) * 6;                     // bytes of this workgroup's pixels that exist
    unsigned char* dst = I.crop + (size_t)e0 * 6;
    for (int k = threadIdx.x; k < n_here / 4; k += 256) reinterpret_cast<unsigned*>(dst)[k] = s_out[k];
    if (threadIdx.x < (n_here & 3)) dst[(n_here & ~3) + threadIdx.x] = reinterpret_cast<unsigned char*>(s_out)[(n_here & ~3) + threadIdx.x];
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
        J.r0 = b[0]; J.c0 = b[1]; J.h = h; J.w = w;
        if (!stored_shape(h, w, J.oh, J.ow)) { J = PatchJob{}; continue; }      // a sliver: nothing to store
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
    if ((rc = Wk.rgb.reserve(n * 3)) || (rc = Wk.color.reserve(n * 12)) || (rc = Wk.depth.reserve(n * 4))) return rc;
    for (int k = 0; k < n_jobs; ++k) HIP_TRY(hipMemcpyAsync(Wk.rgb.as<unsigned char>() + k * HW * 3, rgb[k], HW * 3, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(Wk.color.p, color, n * 12, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(Wk.depth.p, depth, n * 4, hipMemcpyHostToDevice, st));
    const FrameSrc src{Wk.rgb.as<unsigned char>(), Wk.color.as<float>(), Wk.depth.as<float>(), height, width};
    return finish_patches(Wk, st, pj, src, resize_generation, patches);
}

extern "C" int p2p_xyz_rotate_patch_batch(p2p_ctx* ctx, const unsigned char* const* rgb, const float* color, const float* depth, int n_jobs,
                                          int height, int width, const int* n_angles, const double* matrices, const int* rot_shapes,
                                          const float* rgb_table, const float* xyz_table, int resize_generation, unsigned char* patches,
                                          int* shapes)
{
    if (!ctx || n_jobs < 0 || (n_jobs > 0 && (!rgb || !color || !depth || !n_angles || !rgb_table || !xyz_table))) {
        set_error("p2p_xyz_rotate_patch_batch: bad arguments (a null context or buffer)");
        return P2P_ERR_INVALID_ARG;
    }
    if (height <= 0 || width <= 0 || (int64_t)height * width > (1 << 26)) {
        set_error("p2p_xyz_rotate_patch_batch: bad image size %d x %d", height, width);
        return P2P_ERR_INVALID_ARG;
    }
    if (resize_generation != 1) {
        set_error("p2p_xyz_rotate_patch_batch: resize generation %d: only 1 (scikit-image 0.17 / 0.18) is built, the one whose rotate "
                  "is pinned to the real library", resize_generation);
        return P2P_ERR_INVALID_ARG;
    }
    int64_t total = 0;
    for (int k = 0; k < n_jobs; ++k) {
        if (!rgb[k]) {
            set_error("p2p_xyz_rotate_patch_batch: job %d: null frame", k);
            return P2P_ERR_INVALID_ARG;
        }
        if (n_angles[k] < 0 || n_angles[k] > 65535) {
            set_error("p2p_xyz_rotate_patch_batch: job %d: bad angle list (%d angles)", k, n_angles[k]);
            return P2P_ERR_INVALID_ARG;
        }
        total += n_angles[k];
    }
    if (total > 65535 || n_jobs > 65535) {
        set_error("p2p_xyz_rotate_patch_batch: more than 65535 jobs (%d) or angles in all (%lld)", n_jobs, (long long)total);
        return P2P_ERR_INVALID_ARG;
    }
    if (total > 0 && (!matrices || !rot_shapes || !patches || !shapes)) {
        set_error("p2p_xyz_rotate_patch_batch: bad arguments (a null matrix, shape or output buffer)");
        return P2P_ERR_INVALID_ARG;
    }
    for (int q = 0; q < 256; ++q)
        if (!(rgb_table[q] >= 0.f && rgb_table[q] <= 1.f && xyz_table[q] >= 0.f && xyz_table[q] <= 1.f)) {
            set_error("p2p_xyz_rotate_patch_batch: table entry %d outside [0, 1]", q);
            return P2P_ERR_INVALID_ARG;
        }
    const int n_items = (int)total;
    std::vector<RotItem> items(n_items);
    int64_t max_rot = 0;
    for (int k = 0, i = 0; k < n_jobs; ++k)
        for (int a = 0; a < n_angles[k]; ++a, ++i) {
            RotItem& I = items[i];
            I = RotItem{};
            I.job = k; I.rh = rot_shapes[2 * i]; I.rw = rot_shapes[2 * i + 1];
            bool ok = I.rh >= 1 && I.rw >= 1 && I.rh <= height + width + 2 && I.rw <= height + width + 2;
            for (int q = 0; q < 6; ++q) {
                I.m[q] = matrices[6 * i + q];
                ok = ok && std::isfinite(I.m[q]) && std::fabs(I.m[q]) <= 1e6;
            }
            if (!ok) {
                set_error("p2p_xyz_rotate_patch_batch: job %d: bad angle list (entry %d: a matrix that is not finite, or a rotated shape "
                          "%d x %d that no rotation of a %d x %d frame has)", k, a, I.rh, I.rw, height, width);
                return P2P_ERR_INVALID_ARG;
            }
            max_rot = std::max<int64_t>(max_rot, (int64_t)I.rh * I.rw);
            shapes[2 * i] = shapes[2 * i + 1] = 0;
        }
    if (n_items == 0) return P2P_OK;
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    HIP_TRY(hipSetDevice(c->device));
    if (!c->pipe) c->pipe = new Pipeline();
    Pipeline::PatchWork& Wk = c->pipe->patch;
    Pipeline::RotWork& Rk = c->pipe->rot;
    hipStream_t st = c->stream;
    const size_t HW = (size_t)height * width, n = (size_t)n_jobs * HW;
    int rc;
    if ((rc = Wk.rgb.reserve(n * 3)) || (rc = Wk.color.reserve(n * 12)) || (rc = Wk.depth.reserve(n * 4)) || (rc = Rk.lv.reserve(n * 8)) ||
        (rc = Rk.tabs.reserve(512 * 4)) || (rc = Rk.rng.reserve(sizeof(unsigned) * 4 * n_jobs)) ||
        (rc = Rk.items.reserve(sizeof(RotItem) * n_items)) || (rc = Rk.box.reserve(sizeof(int) * 4 * n_items)))
        return rc;
    std::vector<unsigned> rng0((size_t)n_jobs * 4);
    for (int k = 0; k < n_jobs; ++k) { rng0[4 * k] = rng0[4 * k + 2] = ~0u; rng0[4 * k + 1] = rng0[4 * k + 3] = 0u; }
    std::vector<int> box((size_t)n_items * 4);
    for (int i = 0; i < n_items; ++i) { box[4 * i] = box[4 * i + 1] = 0x7fffffff; box[4 * i + 2] = box[4 * i + 3] = -1; }
    // frame and render once per job, whatever the number of its angles
    for (int k = 0; k < n_jobs; ++k) HIP_TRY(hipMemcpyAsync(Wk.rgb.as<unsigned char>() + k * HW * 3, rgb[k], HW * 3, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(Wk.color.p, color, n * 12, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(Wk.depth.p, depth, n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(Rk.tabs.p, rgb_table, 256 * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(Rk.tabs.as<float>() + 256, xyz_table, 256 * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(Rk.rng.p, rng0.data(), sizeof(unsigned) * rng0.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(Rk.items.p, items.data(), sizeof(RotItem) * n_items, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(Rk.box.p, box.data(), sizeof(int) * box.size(), hipMemcpyHostToDevice, st));
    const int lv_blocks = (int)std::min<size_t>(256, (HW + 255) / 256);
    rot_levels_kernel<<<dim3(lv_blocks, n_jobs), 256, 0, st>>>(Wk.rgb.as<unsigned char>(), Wk.color.as<float>(), Wk.depth.as<float>(), (int)HW,
                                                              Rk.tabs.as<float>(), Rk.lv.as<uint2>(), Rk.rng.as<unsigned>());
    HIP_TRY(hipGetLastError());
    rot_mask_box_kernel<<<dim3((unsigned)((max_rot + 255) / 256), n_items), 256, 0, st>>>(Rk.items.as<RotItem>(), Rk.lv.as<uint2>(), height, width,
                                                                                        Rk.box.as<int>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(box.data(), Rk.box.p, sizeof(int) * box.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // the boxes decide the patches' shapes and the size of their crops
    std::vector<PatchJob> pj(n_items);
    std::vector<size_t> crop_off(n_items);
    size_t crop_bytes = 0;
    int max_hw = 0;
    for (int i = 0; i < n_items; ++i) {
        const int* b = &box[4 * i];
        PatchJob& J = pj[i];
        J = PatchJob{};
        if (b[2] < 0) continue;                                           // nothing of the mask is positive: an empty render
        if (b[0] < 0 || b[1] < 0 || b[2] >= items[i].rh || b[3] >= items[i].rw || b[2] < b[0] || b[3] < b[1]) {
            set_error("p2p_xyz_rotate_patch_batch: item %d: box [%d, %d, %d, %d] outside the rotated frame", i, b[0], b[1], b[2], b[3]);
            return P2P_ERR_HIP;
        }
        const int h = b[2] - b[0], w = b[3] - b[1];                       // the max is inclusive and the slice leaves it out
        if (h == 0 || w == 0) continue;
        J.h = h; J.w = w;
        if (!stored_shape(h, w, J.oh, J.ow)) { J = PatchJob{}; continue; }
        items[i].r0 = b[0]; items[i].c0 = b[1]; items[i].h = h; items[i].w = w;
        crop_off[i] = crop_bytes;
        crop_bytes += ((size_t)h * w * 6 + 15) & ~(size_t)15;
        max_hw = std::max(max_hw, h * w);
        shapes[2 * i] = J.oh; shapes[2 * i + 1] = J.ow;
    }
    if ((rc = Rk.crop.reserve(std::max<size_t>(16, crop_bytes)))) return rc;
    for (int i = 0; i < n_items; ++i)
        if (items[i].h) pj[i].crop = items[i].crop = Rk.crop.as<unsigned char>() + crop_off[i];
    if (max_hw > 0) {
        HIP_TRY(hipMemcpyAsync(Rk.items.p, items.data(), sizeof(RotItem) * n_items, hipMemcpyHostToDevice, st));
        rot_patch_kernel<<<dim3((max_hw + 255) / 256, n_items), 256, 0, st>>>(Rk.items.as<RotItem>(), Rk.lv.as<uint2>(), height, width,
                                                                            Rk.tabs.as<float>(), Rk.rng.as<unsigned>());
        HIP_TRY(hipGetLastError());
    }
    return finish_patches(Wk, st, pj, CropSrc{}, resize_generation, patches);
}
