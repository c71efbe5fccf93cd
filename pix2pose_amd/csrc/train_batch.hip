// Training batches (reference pix2pose_util/data_io.py:53-274, get_patch_pair) for scikit-image 0.17 / 0.18: a whole batch in seven
// launches over (sample, tile), from draws the host has already turned into integers.  DESIGN.md section 8.5; tests/train_ref.py
// restates it.  Only the crop window [v1:v2, u1:u2] of the reference's full-frame arrays reaches its outputs, so nothing larger than
// the window (<= 250 x 250) is ever formed: outside the pasted patch image_ref is the background and xyz is 0.5.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "model.h"
#include "pipeline.h"
#include "resize_rules.h"

#pragma clang fp contract(off)

namespace p2p {

namespace {

constexpr int MAXP = P2P_TRAIN_MAX_PATCH;
constexpr int MAXW = P2P_TRAIN_MAX_WINDOW;
constexpr int W2 = MAXW * MAXW;
constexpr int BG_SIDE = 256;      // the staged background: the window, or a whole axis that the enlargement rule stretches (< 2 * 128)
constexpr int MAX_R = 32;         // anti-aliasing radius: sigma = (250 / 16 - 1) / 2 = 7.3 gives 29
constexpr int NCH = 7;            // planes that are rotated and resized: base 3, target 3, mask 1

struct TbSample {
    int ok;
    const unsigned char* patch;       // u8 [ph][pw][pc]
    int ph, pw, pc;
    const unsigned char* bg;          // u8 [bh][bw][3]: rows br0 .. br0 + bh, columns bc0 .. bc0 + bw of the background as loaded
    int bh, bw, br0, bc0;
    int H, W, Hb, Wb;                 // the background as loaded, and the frame (after the enlargement rule)
    int resized;
    float blo, bhi;                   // range of the loaded background (the warp's clip)
    int v_ref, u_ref, v1, u1, wh, ww, D, sv, su;
    int rect[3][4];
    int even;
    int r_edge, r_ran, r_blur, r_aa, r_cblur;
    double w_blur[9], w_ran[5], w_aa[MAX_R + 1];
    float w_cblur[3];
    double rot[6];
    int has_col;
    p2p_train_colour col;
    float* aug;                       // [ph][pw][3] the patch after the colour stage, 0 .. 1
    unsigned char* mk;                // window: bit 0 mask_no_occ_ori, bit 1 mask_no_occ, bit 2 boundary
    float* img;                       // window [3]: image before the blur
    float* imgv;                      // window [3]: its first (row axis) blur pass
    double* cv;                       // window [3]: first pass of the c_img Gaussian (even batches)
    unsigned char* dl;                // window: first pass of the dilations, bit 0 boundary, bit 1 mask_no_occ_ori
    double* base;                     // [D][D][3] base_image
    double* rotb;                     // [D][D][7] rotated base, target, mask
    double* aav;                      // [D][D][7] first pass of the resize's Gaussian
};

__device__ __forceinline__ bool in_rect(const int* r, int Y, int X) { return Y >= r[0] && Y < r[1] && X >= r[2] && X < r[3]; }

// mask_no_occ_ori at a frame pixel: inside the pasted patch and sum(xyz) > 0 (a float32 sum of non-negative terms)
__device__ __forceinline__ bool m_ori(const TbSample& S, int Y, int X)
{
    const int py = Y - S.v_ref, px = X - S.u_ref;
    if (py < 0 || py >= S.ph || px < 0 || px >= S.pw) return false;
    const unsigned char* p = S.patch + ((size_t)py * S.pw + px) * S.pc;
    return (p[3] | p[4] | p[5]) != 0;
}

// c_img = (xyz - 0.5) / 0.5 at a frame pixel whose mask_no_occ_ori is `ori` (elsewhere xyz is 0.5)
__device__ __forceinline__ double c_at(const TbSample& S, int Y, int X, int ch, bool ori)
{
    if (!ori) return 0.0;
    const float f = (float)S.patch[((size_t)(Y - S.v_ref) * S.pw + (X - S.u_ref)) * S.pc + 3 + ch] / 255.0f;
    return ((double)f - 0.5) / 0.5;
}

// the frame's background: float32(u8) / 255, through the float32 warp of resize(order=1, mode='reflect') where it was enlarged
__device__ __forceinline__ float bg_val(const TbSample& S, int Y, int X, int ch)
{
    if (!S.resized) return (float)S.bg[((size_t)(Y - S.br0) * S.bw + (X - S.bc0)) * 3 + ch] / 255.0f;
    const TapF tr = axis_tap_f32(Y, S.H, S.Hb), tc = axis_tap_f32(X, S.W, S.Wb);
    const int r0 = reflect_idx(tr.i0, S.H) - S.br0, r1 = reflect_idx(tr.i1, S.H) - S.br0;
    const int c0 = reflect_idx(tc.i0, S.W) - S.bc0, c1 = reflect_idx(tc.i1, S.W) - S.bc0;
    const float tl = (float)S.bg[((size_t)r0 * S.bw + c0) * 3 + ch] / 255.0f, tp = (float)S.bg[((size_t)r0 * S.bw + c1) * 3 + ch] / 255.0f;
    const float bl = (float)S.bg[((size_t)r1 * S.bw + c0) * 3 + ch] / 255.0f, br = (float)S.bg[((size_t)r1 * S.bw + c1) * 3 + ch] / 255.0f;
    const float w = lerp2_f32(tl, tp, bl, br, tr.d, tc.d);
    return w < S.blo ? S.blo : (w > S.bhi ? S.bhi : w);
}

// ---- colour stage ------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ unsigned long long mix64(unsigned long long z)
{
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// a standard normal keyed by (seed, sample, pixel, channel): two 24-bit uniforms of one mixed word through Box-Muller
__device__ __forceinline__ float keyed_normal(unsigned long long seed, unsigned sample, int pixel, int ch)
{
    const unsigned long long k = mix64(seed ^ mix64(((unsigned long long)sample << 32) | (unsigned)(pixel * 4 + ch)));
    const float u1 = (float)((k >> 40) + 1ull) * (1.0f / 16777216.0f);
    const float u2 = (float)((k >> 8) & 0xffffffull) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

__device__ __forceinline__ float clip255(float v) { return v < 0.f ? 0.f : (v > 255.f ? 255.f : v); }

// the point-wise augmenters order[from .. to) on one pixel's 0 .. 255 values, clipped after each
__device__ inline void colour_ops(const p2p_train_colour& c, int from, int to, int pixel, float x[3])
{
    for (int k = from; k < to; ++k) {
        const int id = c.order[k];
        if (id < 3) x[id] = x[id] + c.add[id];
        else if (id == 3) { for (int ch = 0; ch < 3; ++ch) x[ch] = 128.f + c.contrast * (x[ch] - 128.f); }
        else if (id == 4) { for (int ch = 0; ch < 3; ++ch) x[ch] = x[ch] * c.mul[ch]; }
        else if (id == 6) {
            if (c.noise_scale > 0.f)
                for (int ch = 0; ch < 3; ++ch) x[ch] = x[ch] + c.noise_scale * keyed_normal(c.seed, c.sample, pixel, ch);
        } else if (id == 7) { for (int ch = 0; ch < 3; ++ch) x[ch] = 128.f + c.contrast2[ch] * (x[ch] - 128.f); }
        for (int ch = 0; ch < 3; ++ch) x[ch] = clip255(x[ch]);
    }
}

// One thread per patch pixel: img_augmented = seq_syn(real_img * 255) / 255 (:87), real_img = float32(u8) / 255.  The blur (radius <= 2,
// mirrored edges) reads neighbours on which the augmenters before it are applied again: they are point-wise and the noise is keyed
// by the pixel, so no second buffer and no second launch is needed.
__global__ void __launch_bounds__(256) tb_colour_kernel(const TbSample* __restrict__ samples)
{
    const TbSample& S = samples[blockIdx.y];
    if (!S.ok) return;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= S.ph * S.pw) return;
    const int py = p / S.pw, px = p - py * S.pw;
    float x[3];
    if (!S.has_col) {
        for (int ch = 0; ch < 3; ++ch) x[ch] = ((float)S.patch[(size_t)p * S.pc + ch] / 255.0f) * 255.0f;
    } else {
        int b = 8;
        for (int k = 0; k < 8; ++k) if (S.col.order[k] == 5) b = k;
        if (S.r_cblur == 0 || b == 8) {
            for (int ch = 0; ch < 3; ++ch) x[ch] = ((float)S.patch[(size_t)p * S.pc + ch] / 255.0f) * 255.0f;
            colour_ops(S.col, 0, 8, p, x);
        } else {
            float acc[3] = {0.f, 0.f, 0.f};
            for (int dy = -S.r_cblur; dy <= S.r_cblur; ++dy)
                for (int dx = -S.r_cblur; dx <= S.r_cblur; ++dx) {
                    const int q = reflect_idx(py + dy, S.ph) * S.pw + reflect_idx(px + dx, S.pw);
                    float v[3];
                    for (int ch = 0; ch < 3; ++ch) v[ch] = ((float)S.patch[(size_t)q * S.pc + ch] / 255.0f) * 255.0f;
                    colour_ops(S.col, 0, b, q, v);
                    const float w = S.w_cblur[dy < 0 ? -dy : dy] * S.w_cblur[dx < 0 ? -dx : dx];
                    for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + w * v[ch];
                }
            for (int ch = 0; ch < 3; ++ch) x[ch] = clip255(acc[ch]);
            colour_ops(S.col, b + 1, 8, p, x);
        }
    }
    for (int ch = 0; ch < 3; ++ch) S.aug[(size_t)p * 3 + ch] = x[ch] / 255.0f;
}

// ---- window stages -----------------------------------------------------------------------------------------------------------------

// One thread per window pixel: the masks, the boundary (np.gradient of the window's mask_no_occ: central differences inside, one-sided
// at the window's edges; only their sign is used) and `image` = image_ref under mask_no_occ, the background elsewhere (:172, :186).
__global__ void __launch_bounds__(256) tb_compose_kernel(const TbSample* __restrict__ samples)
{
    const TbSample& S = samples[blockIdx.y];
    if (!S.ok) return;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= S.wh * S.ww) return;
    const int y = p / S.ww, x = p - y * S.ww;
    const int Y = S.v1 + y, X = S.u1 + x;
    auto mno = [&](int yy, int xx) { return (m_ori(S, S.v1 + yy, S.u1 + xx) && !in_rect(S.rect[0], S.v1 + yy, S.u1 + xx)) ? 1 : 0; };
    const bool ori = m_ori(S, Y, X);
    const bool no = ori && !in_rect(S.rect[0], Y, X);
    const int gy = y == 0 ? mno(1, x) - mno(0, x) : (y == S.wh - 1 ? mno(y, x) - mno(y - 1, x) : mno(y + 1, x) - mno(y - 1, x));
    const int gx = x == 0 ? mno(y, 1) - mno(y, 0) : (x == S.ww - 1 ? mno(y, x) - mno(y, x - 1) : mno(y, x + 1) - mno(y, x - 1));
    S.mk[p] = (unsigned char)((ori ? 1 : 0) | (no ? 2 : 0) | ((gy > 0 || gx > 0) ? 4 : 0));
    for (int ch = 0; ch < 3; ++ch)
        S.img[(size_t)p * 3 + ch] = no ? S.aug[((size_t)(Y - S.v_ref) * S.pw + (X - S.u_ref)) * 3 + ch] : bg_val(S, Y, X, ch);
}

// First (row axis) pass of everything separable, one thread per window pixel.  The two thresholded Gaussians (:192, :207-208) are
// square dilations: every weight of scipy's kernel is positive, so the filtered value is > 0 exactly where a pixel of the
// (2 r + 1)^2 neighbourhood is set, r = int(4 sigma + 0.5); mode='nearest' repeats pixels that the neighbourhood already holds.
// The image blur keeps scipy's float32 array between the passes; the c_img Gaussian is float64.
__global__ void __launch_bounds__(256) tb_vpass_kernel(const TbSample* __restrict__ samples)
{
    const TbSample& S = samples[blockIdx.y];
    if (!S.ok) return;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= S.wh * S.ww) return;
    const int y = p / S.ww, x = p - y * S.ww;
    int e = 0, o = 0;
    for (int dy = -S.r_edge; dy <= S.r_edge; ++dy) {
        const int yy = y + dy;
        if (yy >= 0 && yy < S.wh) e |= (S.mk[yy * S.ww + x] >> 2) & 1;
    }
    double b[3] = {0.0, 0.0, 0.0};
    for (int dy = -S.r_blur; dy <= S.r_blur; ++dy) {
        const int yy = min(max(y + dy, 0), S.wh - 1);
        const double w = S.w_blur[dy < 0 ? -dy : dy];
        for (int ch = 0; ch < 3; ++ch) b[ch] = b[ch] + w * (double)S.img[((size_t)yy * S.ww + x) * 3 + ch];
    }
    for (int ch = 0; ch < 3; ++ch) S.imgv[(size_t)p * 3 + ch] = (float)b[ch];
    if (S.even) {
        double c[3] = {0.0, 0.0, 0.0};
        for (int dy = -S.r_ran; dy <= S.r_ran; ++dy) {
            const int yy = y + dy;
            if (yy >= 0 && yy < S.wh) o |= S.mk[yy * S.ww + x] & 1;
            const int yc = min(max(yy, 0), S.wh - 1);
            const bool ori = S.mk[yc * S.ww + x] & 1;
            const double w = S.w_ran[dy < 0 ? -dy : dy];
            for (int ch = 0; ch < 3; ++ch) c[ch] = c[ch] + w * c_at(S, S.v1 + yc, S.u1 + x, ch, ori);
        }
        for (int ch = 0; ch < 3; ++ch) S.cv[(size_t)p * 3 + ch] = c[ch];
    }
    S.dl[p] = (unsigned char)(e | (o << 1));
}

// Second pass and everything point-wise behind it, one thread per pixel of base_image [D][D]: the blurred boundary (:195), on even
// batches the grey-out by the dilated mask and radius > 0.3 (double), the second occlusion and the background inclusion (:203-250),
// the normalisation and the placement (:259).  Pixels outside the clipped window are 0.
__global__ void __launch_bounds__(256) tb_hpass_kernel(const TbSample* __restrict__ samples)
{
    const TbSample& S = samples[blockIdx.y];
    if (!S.ok) return;
    const int pb = blockIdx.x * 256 + threadIdx.x;
    if (pb >= S.D * S.D) return;
    const int yb = pb / S.D, xb = pb - yb * S.D;
    const int y = yb - S.sv, x = xb - S.su;
    double* out = S.base + (size_t)pb * 3;
    if (y < 0 || y >= S.wh || x < 0 || x >= S.ww) { out[0] = out[1] = out[2] = 0.0; return; }
    const int p = y * S.ww + x;
    const int Y = S.v1 + y, X = S.u1 + x;
    int e = 0;
    for (int dx = -S.r_edge; dx <= S.r_edge; ++dx) {
        const int xx = x + dx;
        if (xx >= 0 && xx < S.ww) e |= S.dl[y * S.ww + xx] & 1;
    }
    float v[3];
    if (e) {
        double b[3] = {0.0, 0.0, 0.0};
        for (int dx = -S.r_blur; dx <= S.r_blur; ++dx) {
            const int xx = min(max(x + dx, 0), S.ww - 1);
            const double w = S.w_blur[dx < 0 ? -dx : dx];
            for (int ch = 0; ch < 3; ++ch) b[ch] = b[ch] + w * (double)S.imgv[((size_t)y * S.ww + xx) * 3 + ch];
        }
        for (int ch = 0; ch < 3; ++ch) v[ch] = (float)b[ch];
    } else {
        for (int ch = 0; ch < 3; ++ch) v[ch] = S.img[(size_t)p * 3 + ch];
    }
    if (S.even) {
        int o = 0;
        double c[3] = {0.0, 0.0, 0.0};
        for (int dx = -S.r_ran; dx <= S.r_ran; ++dx) {
            const int xx = x + dx;
            if (xx >= 0 && xx < S.ww) o |= (S.dl[y * S.ww + xx] >> 1) & 1;
            const int xc = min(max(xx, 0), S.ww - 1);
            const double w = S.w_ran[dx < 0 ? -dx : dx];
            for (int ch = 0; ch < 3; ++ch) c[ch] = c[ch] + w * S.cv[((size_t)y * S.ww + xc) * 3 + ch];
        }
        const double radius = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        if (!(o && radius > 0.3)) v[0] = v[1] = v[2] = 0.5f;
        if (in_rect(S.rect[1], Y, X)) v[0] = v[1] = v[2] = 0.5f;
        if (in_rect(S.rect[2], Y, X) && !(S.mk[p] & 1))
            for (int ch = 0; ch < 3; ++ch) v[ch] = bg_val(S, Y, X, ch);      // image_ref off the object is the background
    }
    for (int ch = 0; ch < 3; ++ch) out[ch] = ((double)v[ch] - 0.5) / 0.5;
}

// tgt_image and mask_image at a pixel of the [D][D] canvas (:261-262): c_img and mask_no_occ_ori inside the window, 0 outside
__device__ __forceinline__ void canvas_tgt(const TbSample& S, int yb, int xb, double t[4])
{
    const int y = yb - S.sv, x = xb - S.su;
    t[0] = t[1] = t[2] = t[3] = 0.0;
    if (y < 0 || y >= S.wh || x < 0 || x >= S.ww) return;
    if (!(S.mk[y * S.ww + x] & 1)) return;
    for (int ch = 0; ch < 3; ++ch) t[ch] = c_at(S, S.v1 + y, S.u1 + x, ch, true);
    t[3] = 1.0;
}

// rotate(angle) of the three canvases without resize (:265-268), one thread per output pixel, everything in double: base and
// target with mode='reflect', the mask with mode='constant', cval 0.  The library's clip to the input's range is not applied: the
// taps' weights are non-negative and sum to 1, so it can only move a value by the rounding of that sum.
__global__ void __launch_bounds__(256) tb_rotate_kernel(const TbSample* __restrict__ samples)
{
    const TbSample& S = samples[blockIdx.y];
    if (!S.ok) return;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int D = S.D;
    if (p >= D * D) return;
    const int oy = p / D, ox = p - oy * D;
    const double x = (double)ox, y = (double)oy;
    const double c = S.rot[0] * x + S.rot[1] * y + S.rot[2];
    const double r = S.rot[3] * x + S.rot[4] * y + S.rot[5];
    const double fr = floor(r), fc = floor(c);
    const int minr = (int)fr, minc = (int)fc, maxr = (int)ceil(r), maxc = (int)ceil(c);
    const double dr = r - fr, dc = c - fc;
    const int rr[2] = {reflect_idx(minr, D), reflect_idx(maxr, D)};
    const int cc[2] = {reflect_idx(minc, D), reflect_idx(maxc, D)};
    const int cr[2] = {minr, maxr}, cq[2] = {minc, maxc};
    double t[2][2][4], m[2][2];
    for (int a = 0; a < 2; ++a)
        for (int e = 0; e < 2; ++e) {
            canvas_tgt(S, rr[a], cc[e], t[a][e]);
            double u[4] = {0.0, 0.0, 0.0, 0.0};
            if (cr[a] >= 0 && cr[a] < D && cq[e] >= 0 && cq[e] < D) canvas_tgt(S, cr[a], cq[e], u);
            m[a][e] = u[3];
        }
    double* out = S.rotb + (size_t)p * NCH;
    for (int ch = 0; ch < 3; ++ch) {
        const double* b = S.base + ch;
        out[ch] = lerp2(b[((size_t)rr[0] * D + cc[0]) * 3], b[((size_t)rr[0] * D + cc[1]) * 3], b[((size_t)rr[1] * D + cc[0]) * 3],
                        b[((size_t)rr[1] * D + cc[1]) * 3], dr, dc);
        out[3 + ch] = lerp2(t[0][0][ch], t[0][1][ch], t[1][0][ch], t[1][1][ch], dr, dc);
    }
    out[6] = lerp2(m[0][0], m[0][1], m[1][0], m[1][1], dr, dc);
}

// resize's Gaussian pre-filter (D > imsize), row axis, mode 'mirror'; one thread per canvas pixel, seven planes
__global__ void __launch_bounds__(256) tb_aa_vpass_kernel(const TbSample* __restrict__ samples)
{
    const TbSample& S = samples[blockIdx.y];
    if (!S.ok || S.r_aa == 0) return;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int D = S.D;
    if (p >= D * D) return;
    const int y = p / D, x = p - y * D;
    double acc[NCH] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int dy = -S.r_aa; dy <= S.r_aa; ++dy) {
        const double w = S.w_aa[dy < 0 ? -dy : dy];
        const double* src = S.rotb + ((size_t)reflect_idx(y + dy, D) * D + x) * NCH;
        for (int k = 0; k < NCH; ++k) acc[k] = acc[k] + w * src[k];
    }
    for (int k = 0; k < NCH; ++k) S.aav[(size_t)p * NCH + k] = acc[k];
}

// resize(..., (imsize, imsize), order=1, mode='reflect') of the three rotated canvases (:270-272) in double, one thread per output
// pixel: the column pass of the pre-filter is taken at the four taps, then the bilinear rule of resize_rules.h.  Unclipped, as above.
__global__ void __launch_bounds__(256) tb_resize_kernel(const TbSample* __restrict__ samples, int imsize, float* __restrict__ src,
                                                        float* __restrict__ tgt, float* __restrict__ mask)
{
    const TbSample& S = samples[blockIdx.y];
    if (!S.ok) return;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= imsize * imsize) return;
    const int oy = p / imsize, ox = p - oy * imsize;
    const int D = S.D;
    const Tap tr = axis_tap(oy, D, imsize), tc = axis_tap(ox, D, imsize);
    const int rr[2] = {reflect_idx(tr.i0, D), reflect_idx(tr.i1, D)};
    const int cc[2] = {reflect_idx(tc.i0, D), reflect_idx(tc.i1, D)};
    double v[2][2][NCH];
    for (int a = 0; a < 2; ++a)
        for (int e = 0; e < 2; ++e) {
            if (S.r_aa == 0) {
                const double* q = S.rotb + ((size_t)rr[a] * D + cc[e]) * NCH;
                for (int k = 0; k < NCH; ++k) v[a][e][k] = q[k];
            } else {
                for (int k = 0; k < NCH; ++k) v[a][e][k] = 0.0;
                for (int dx = -S.r_aa; dx <= S.r_aa; ++dx) {
                    const double w = S.w_aa[dx < 0 ? -dx : dx];
                    const double* q = S.aav + ((size_t)rr[a] * D + reflect_idx(cc[e] + dx, D)) * NCH;
                    for (int k = 0; k < NCH; ++k) v[a][e][k] = v[a][e][k] + w * q[k];
                }
            }
        }
    const size_t o = (size_t)blockIdx.y * imsize * imsize + p;
    for (int ch = 0; ch < 3; ++ch) {
        src[o * 3 + ch] = (float)lerp2(v[0][0][ch], v[0][1][ch], v[1][0][ch], v[1][1][ch], tr.d, tc.d);
        tgt[o * 3 + ch] = (float)lerp2(v[0][0][3 + ch], v[0][1][3 + ch], v[1][0][3 + ch], v[1][1][3 + ch], tr.d, tc.d);
    }
    mask[o] = (float)lerp2(v[0][0][6], v[0][1][6], v[1][0][6], v[1][1][6], tr.d, tc.d);
}

// scipy.ndimage's Gaussian kernel, one-sided (centre first): radius int(4 sigma + 0.5), exp(-0.5 x^2 / sigma^2) over its sum
int gauss_weights(double sigma, double* w)
{
    const int radius = sigma > 1e-15 ? (int)(4.0 * sigma + 0.5) : 0;
    if (radius == 0) { w[0] = 1.0; return 0; }
    const double c = -0.5 / (sigma * sigma);
    double s = 0.0;
    for (int x = -radius; x <= radius; ++x) s += std::exp(c * (double)(x * x));
    for (int d = 0; d <= radius; ++d) w[d] = std::exp(c * (double)(d * d)) / s;
    return radius;
}

bool rect_ok(const int* r, int Hb, int Wb)
{
    if (r[0] >= r[1] || r[2] >= r[3]) return true;      // none
    return r[0] >= 0 && r[1] <= Hb && r[2] >= 0 && r[3] <= Wb;
}

}  // namespace

}  // namespace p2p

using namespace p2p;

extern "C" int p2p_train_sizeof(int which)
{
    return which == 0 ? (int)sizeof(p2p_train_draw) : (which == 1 ? (int)sizeof(p2p_train_colour) : -1);
}

extern "C" int p2p_train_batch(p2p_ctx* ctx, int n, const unsigned char* const* patches, const int* patch_shapes,
                               const unsigned char* const* backgrounds, const int* back_shapes, const p2p_train_draw* draws,
                               const p2p_train_colour* colours, int imsize, int generation, float* src, float* tgt, float* mask, int out_mem,
                               int* status)
{
    if (!ctx || n < 0 || n > 65535 || (n > 0 && (!patches || !patch_shapes || !backgrounds || !back_shapes || !draws || !src || !tgt || !mask || !status))) {
        set_error("p2p_train_batch: bad arguments (a null context or buffer, or more than 65535 samples)");
        return P2P_ERR_INVALID_ARG;
    }
    if (imsize < 16 || imsize > 512 || (out_mem != P2P_MEM_HOST && out_mem != P2P_MEM_DEVICE)) {
        set_error("p2p_train_batch: imsize %d outside 16 .. 512, or a bad out_mem %d", imsize, out_mem);
        return P2P_ERR_INVALID_ARG;
    }
    if (generation != 1) {
        set_error("p2p_train_batch: resize generation %d: only 1 (scikit-image 0.17 / 0.18) is built, the one the fixtures were "
                  "recorded with", generation);
        return P2P_ERR_INVALID_ARG;
    }
    if (n == 0) return P2P_OK;
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    HIP_TRY(hipSetDevice(c->device));
    if (!c->pipe) c->pipe = new Pipeline();
    Pipeline::TrainWork& Wk = c->pipe->train;
    hipStream_t st = c->stream;

    constexpr size_t PATCH_SLOT = (size_t)MAXP * MAXP * 7, BG_SLOT = (size_t)BG_SIDE * BG_SIDE * 3;
    const size_t out_px = (size_t)n * imsize * imsize;
    int rc;
    if ((rc = Wk.samples.reserve(sizeof(TbSample) * n)) || (rc = Wk.patch.reserve(PATCH_SLOT * n)) || (rc = Wk.bg.reserve(BG_SLOT * n)) ||
        (rc = Wk.aug.reserve((size_t)n * MAXP * MAXP * 3 * 4)) || (rc = Wk.mk.reserve((size_t)n * W2)) || (rc = Wk.img.reserve((size_t)n * W2 * 12)) ||
        (rc = Wk.imgv.reserve((size_t)n * W2 * 12)) || (rc = Wk.cv.reserve((size_t)n * W2 * 24)) || (rc = Wk.dl.reserve((size_t)n * W2)) ||
        (rc = Wk.base.reserve((size_t)n * W2 * 24)) || (rc = Wk.rot.reserve((size_t)n * W2 * NCH * 8)) ||
        (rc = Wk.aav.reserve((size_t)n * W2 * NCH * 8)) || (rc = Wk.stage.reserve((PATCH_SLOT + BG_SLOT) * n)))
        return rc;
    if (out_mem == P2P_MEM_HOST && ((rc = Wk.out.reserve(out_px * 7 * 4)) || (rc = Wk.h_out.reserve(out_px * 7 * 4)))) return rc;

    // the stream may still read the staging buffer of the previous call's copies only until that call returned (it synchronises)
    unsigned char* h_patch = Wk.stage.as<unsigned char>();
    unsigned char* h_bg = h_patch + PATCH_SLOT * n;
    std::vector<TbSample> hs(n);
    std::vector<double> waa;
    bool named = false;
    int max_patch = 0, max_win = 0, max_side = 0, n_ok = 0;
    bool any_aa = false;
    for (int k = 0; k < n; ++k) {
        TbSample& S = hs[k];
        std::memset(&S, 0, sizeof(S));
        const int* ps = patch_shapes + 3 * k;
        const int* bs = back_shapes + 3 * k;
        const p2p_train_draw& d = draws[k];
        auto fail = [&](int code, const char* why) {
            status[k] = code;
            if (!named) { set_error("p2p_train_batch: sample %d: %s", k, why); named = true; }
        };
        status[k] = P2P_TRAIN_OK;
        if (!patches[k] || (ps[2] != 6 && ps[2] != 7) || ps[0] < 1 || ps[1] < 1 || ps[0] > MAXP || ps[1] > MAXP) {
            fail(P2P_TRAIN_BAD_PATCH, "bad patch (null, not 6 or 7 channels, or a side outside 1 .. 128)");
            continue;
        }
        const int ph = ps[0], pw = ps[1], H = bs[0], W = bs[1];
        if (!backgrounds[k] || (bs[2] != 1 && bs[2] != 3) || H < 1 || W < 1 || H > 32768 || W > 32768) {
            fail(P2P_TRAIN_BAD_BACKGROUND, "bad background (null, not 1 or 3 channels, or a side outside 1 .. 32768)");
            continue;
        }
        const bool resized = H < 2 * ph || W < 2 * pw;
        const int Hb = resized ? std::max(H < 2 * ph ? 2 * ph : 0, H) : H, Wb = resized ? std::max(W < 2 * pw ? 2 * pw : 0, W) : W;
        if (Hb < ph + 20 || Wb < pw + 20) {
            fail(P2P_TRAIN_BAD_BACKGROUND, "background smaller than the patch plus 20 after the enlargement rule");
            continue;
        }
        bool ok = std::isfinite(d.sigma_edge) && std::isfinite(d.sigma_blur) && d.sigma_edge >= 0 && d.sigma_edge <= 2 && d.sigma_blur >= 0 &&
                  d.sigma_blur <= 2;
        if (d.even) ok = ok && std::isfinite(d.sigma_ran) && d.sigma_ran >= 0.1 && d.sigma_ran <= 1.0;
        for (int q = 0; q < 6; ++q) ok = ok && std::isfinite(d.rot[q]) && std::fabs(d.rot[q]) <= 1e5;
        if (!ok) {
            fail(P2P_TRAIN_BAD_DRAW, "a sigma or rotation entry that is not finite or outside its range");
            continue;
        }
        const int wh = d.v2 - d.v1, ww = d.u2 - d.u1;
        ok = d.v_ref >= 0 && d.u_ref >= 0 && d.v_ref + ph <= Hb && d.u_ref + pw <= Wb && d.v1 >= 0 && d.u1 >= 0 && d.v2 <= Hb && d.u2 <= Wb &&
             wh >= 2 && ww >= 2 && d.side >= 2 && d.side <= MAXW && d.shift_v >= 0 && d.shift_u >= 0 && d.shift_v + wh <= d.side &&
             d.shift_u + ww <= d.side;
        for (int q = 0; q < 3; ++q) ok = ok && rect_ok(d.rect[q], Hb, Wb);
        if (!ok) {
            fail(P2P_TRAIN_BAD_DRAW, "paste position, window or rectangle outside the frame, or a window above 250");
            continue;
        }
        S.ok = 1;
        S.ph = ph; S.pw = pw; S.pc = ps[2];
        S.H = H; S.W = W; S.Hb = Hb; S.Wb = Wb; S.resized = resized ? 1 : 0;
        S.v_ref = d.v_ref; S.u_ref = d.u_ref; S.v1 = d.v1; S.u1 = d.u1; S.wh = wh; S.ww = ww; S.D = d.side; S.sv = d.shift_v; S.su = d.shift_u;
        std::memcpy(S.rect, d.rect, sizeof(S.rect));
        S.even = d.even ? 1 : 0;
        S.r_edge = d.sigma_edge > 1e-15 ? (int)(4.0 * d.sigma_edge + 0.5) : 0;
        S.r_blur = gauss_weights(d.sigma_blur, S.w_blur);
        S.r_ran = S.even ? gauss_weights(d.sigma_ran, S.w_ran) : 0;
        S.r_aa = aa_weights_for_axis(S.D, imsize, waa);
        if (S.r_aa > MAX_R) { S.ok = 0; fail(P2P_TRAIN_BAD_DRAW, "anti-aliasing radius above the bound"); continue; }
        for (int q = 0; q <= S.r_aa && S.r_aa > 0; ++q) S.w_aa[q] = waa[q];
        any_aa = any_aa || S.r_aa > 0;
        std::memcpy(S.rot, d.rot, sizeof(S.rot));
        if (colours) {
            const p2p_train_colour& col = colours[k];
            int seen = 0;
            for (int q = 0; q < 8; ++q) if (col.order[q] >= 0 && col.order[q] < 8) seen |= 1 << col.order[q];
            bool cok = seen == 255 && std::isfinite(col.contrast) && std::isfinite(col.blur_sigma) && col.blur_sigma >= 0.f && col.blur_sigma <= 0.5f &&
                       std::isfinite(col.noise_scale) && col.noise_scale >= 0.f;
            for (int q = 0; q < 3; ++q) cok = cok && std::isfinite(col.add[q]) && std::isfinite(col.mul[q]) && std::isfinite(col.contrast2[q]);
            if (!cok) { S.ok = 0; fail(P2P_TRAIN_BAD_DRAW, "colour record: order is no permutation, or a parameter not finite or out of range"); continue; }
            S.has_col = 1; S.col = col;
            double wc[9];
            S.r_cblur = gauss_weights((double)col.blur_sigma, wc);
            for (int q = 0; q <= S.r_cblur; ++q) S.w_cblur[q] = (float)wc[q];
        }
        // stage the patch, and of the background what the window reads: the window itself, or along an axis that is stretched the whole axis
        std::memcpy(h_patch + PATCH_SLOT * k, patches[k], (size_t)ph * pw * S.pc);
        const bool rows_all = resized && H != Hb, cols_all = resized && W != Wb;
        S.br0 = rows_all ? 0 : d.v1; S.bh = rows_all ? H : wh;
        S.bc0 = cols_all ? 0 : d.u1; S.bw = cols_all ? W : ww;
        const int C = bs[2];
        unsigned char* dst = h_bg + BG_SLOT * k;
        for (int r = 0; r < S.bh; ++r) {
            const unsigned char* srow = backgrounds[k] + ((size_t)(S.br0 + r) * W + S.bc0) * C;
            if (C == 3) std::memcpy(dst + (size_t)r * S.bw * 3, srow, (size_t)S.bw * 3);
            else for (int q = 0; q < S.bw; ++q) dst[((size_t)r * S.bw + q) * 3] = dst[((size_t)r * S.bw + q) * 3 + 1] = dst[((size_t)r * S.bw + q) * 3 + 2] = srow[q];
        }
        if (resized) {
            unsigned char lo = 255, hi = 0;
            const size_t cnt = (size_t)H * W * C;
            for (size_t q = 0; q < cnt; ++q) { lo = std::min(lo, backgrounds[k][q]); hi = std::max(hi, backgrounds[k][q]); }
            S.blo = (float)lo / 255.0f; S.bhi = (float)hi / 255.0f;
        }
        S.patch = Wk.patch.as<unsigned char>() + PATCH_SLOT * k;
        S.bg = Wk.bg.as<unsigned char>() + BG_SLOT * k;
        S.aug = Wk.aug.as<float>() + (size_t)k * MAXP * MAXP * 3;
        S.mk = Wk.mk.as<unsigned char>() + (size_t)k * W2;
        S.img = Wk.img.as<float>() + (size_t)k * W2 * 3;
        S.imgv = Wk.imgv.as<float>() + (size_t)k * W2 * 3;
        S.cv = Wk.cv.as<double>() + (size_t)k * W2 * 3;
        S.dl = Wk.dl.as<unsigned char>() + (size_t)k * W2;
        S.base = Wk.base.as<double>() + (size_t)k * W2 * 3;
        S.rotb = Wk.rot.as<double>() + (size_t)k * W2 * NCH;
        S.aav = Wk.aav.as<double>() + (size_t)k * W2 * NCH;
        max_patch = std::max(max_patch, ph * pw); max_win = std::max(max_win, wh * ww); max_side = std::max(max_side, S.D * S.D);
        ++n_ok;
    }
    float* d_src = out_mem == P2P_MEM_DEVICE ? src : Wk.out.as<float>();
    float* d_tgt = out_mem == P2P_MEM_DEVICE ? tgt : d_src + out_px * 3;
    float* d_mask = out_mem == P2P_MEM_DEVICE ? mask : d_tgt + out_px * 3;
    HIP_TRY(hipMemsetAsync(d_src, 0, out_px * 12, st));
    HIP_TRY(hipMemsetAsync(d_tgt, 0, out_px * 12, st));
    HIP_TRY(hipMemsetAsync(d_mask, 0, out_px * 4, st));
    if (n_ok > 0) {
        HIP_TRY(hipMemcpyAsync(Wk.patch.p, h_patch, PATCH_SLOT * n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(Wk.bg.p, h_bg, BG_SLOT * n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(Wk.samples.p, hs.data(), sizeof(TbSample) * n, hipMemcpyHostToDevice, st));
        const TbSample* ds = Wk.samples.as<TbSample>();
        tb_colour_kernel<<<dim3((max_patch + 255) / 256, n), 256, 0, st>>>(ds);
        HIP_TRY(hipGetLastError());
        tb_compose_kernel<<<dim3((max_win + 255) / 256, n), 256, 0, st>>>(ds);
        HIP_TRY(hipGetLastError());
        tb_vpass_kernel<<<dim3((max_win + 255) / 256, n), 256, 0, st>>>(ds);
        HIP_TRY(hipGetLastError());
        tb_hpass_kernel<<<dim3((max_side + 255) / 256, n), 256, 0, st>>>(ds);
        HIP_TRY(hipGetLastError());
        tb_rotate_kernel<<<dim3((max_side + 255) / 256, n), 256, 0, st>>>(ds);
        HIP_TRY(hipGetLastError());
        if (any_aa) {
            tb_aa_vpass_kernel<<<dim3((max_side + 255) / 256, n), 256, 0, st>>>(ds);
            HIP_TRY(hipGetLastError());
        }
        tb_resize_kernel<<<dim3((imsize * imsize + 255) / 256, n), 256, 0, st>>>(ds, imsize, d_src, d_tgt, d_mask);
        HIP_TRY(hipGetLastError());
    }
    if (out_mem == P2P_MEM_HOST) HIP_TRY(hipMemcpyAsync(Wk.h_out.p, Wk.out.p, out_px * 7 * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (out_mem == P2P_MEM_HOST) {
        const float* h = Wk.h_out.as<float>();
        std::memcpy(src, h, out_px * 12);
        std::memcpy(tgt, h + out_px * 3, out_px * 12);
        std::memcpy(mask, h + out_px * 6, out_px * 4);
    }
    return P2P_OK;
}
