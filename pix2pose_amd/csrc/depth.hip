// Depth path of the RGB-D evaluation (reference tools/5_evaluation_bop_icp3d.py): meshes in HBM, a depth-only z-buffer
// (render_obj(), :40-50, through rendering/renderer_xyz.py) and the depth-agreement score of a detection (:470-490).
// The exact rules (projection, coverage, ties, clipping, culling) are written down in DESIGN.md section 8; tests/depth_ref.py
// restates them in float64 numpy.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "model.h"
#include "pipeline.h"

#pragma clang fp contract(off)     // no FMA contraction: the restatement evaluates the same expressions in the same order

struct p2p_mesh {
    int device = 0;
    int n_verts = 0, n_tris = 0;
    float* verts = nullptr;   // [n_verts][3] metres (float32, like Model3D.load(scale=0.001))
    int* tris = nullptr;      // [n_tris][3], every index checked against n_verts at creation
    float* colors = nullptr;  // [n_verts][3] float32(c) / 255 (p2p_mesh_set_colors), null until set
};

namespace p2p {

namespace {

constexpr double CLIP_NEAR = 0.01, CLIP_FAR = 10.0;      // Renderer.set_cam defaults (renderer_xyz.py:126)
constexpr unsigned DEPTH_EMPTY = 0x7f800000u;            // +inf: above every finite depth in the atomicMin order of positive floats
// Winner key of the colour path: (depth bits << 32) | triangle index, so atomicMin keeps the nearest fragment and, among fragments
// of equal float32 depth, the lowest triangle index.  All ones (what a byte memset writes) is above every key of a drawn fragment.
typedef unsigned long long WinnerKey;
constexpr WinnerKey KEY_EMPTY = ~0ull;
constexpr int RASTER_THREADS = 256, SCORE_THREADS = 256;

// One job as the device sees it: the mesh's arrays, the pose in metres (unit quirk applied), the intrinsics.
struct RasterJob {
    const float* verts;
    const int* tris;
    int n_tris;
    double R[9], t[3];
    double fx, s, cx, fy, cy;
    const float* colors;      // colour path only
};

// Edge function of a -> b at p, and the owner rule for a sample exactly on the edge: with the triangle ordered so that
// its area is positive, an edge owns its ties when it runs towards +v, or along v = const towards -u.  The two triangles sharing an
// edge traverse it in opposite directions, so exactly one of them owns a tie.
__device__ __forceinline__ double edge_fn(double au, double av, double bu, double bv, double pu, double pv)
{
    return (bu - au) * (pv - av) - (bv - av) * (pu - au);
}
__device__ __forceinline__ bool edge_in(double e, double au, double av, double bu, double bv)
{
    const double dv = bv - av, du = bu - au;
    return e > 0.0 || (e == 0.0 && (dv > 0.0 || (dv == 0.0 && du < 0.0)));
}

// Triangle set-up shared by both routes: project, cull, clip; on success the vertices are ordered for a positive area A and
// [i0, i1] x [j0, j1] is the pixel box clamped to the image (every index formed from it is in bounds).
struct TriSetup {
    double u[3], v[3], z[3], A;
    int i0, i1, j0, j1;
};

__device__ __forceinline__ bool tri_setup(const RasterJob& J, int f, int H, int W, TriSetup& T)
{
    for (int k = 0; k < 3; ++k) {
        const float* p = J.verts + 3 * (size_t)J.tris[3 * (size_t)f + k];
        const double X = p[0], Y = p[1], Z = p[2];
        const double xc = J.R[0] * X + J.R[1] * Y + J.R[2] * Z + J.t[0];
        const double yc = J.R[3] * X + J.R[4] * Y + J.R[5] * Z + J.t[1];
        const double zc = J.R[6] * X + J.R[7] * Y + J.R[8] * Z + J.t[2];
        if (!(zc >= CLIP_NEAR)) return false;      // straddles / lies before the near plane (or NaN): rejected whole
        T.u[k] = J.fx * (xc / zc) + J.s * (yc / zc) + J.cx;
        T.v[k] = J.fy * (yc / zc) + J.cy;
        T.z[k] = zc;
        if (!(fabs(T.u[k]) < 1e9 && fabs(T.v[k]) < 1e9)) return false;
    }
    // front faces have a negative area in (u, v) (v down): counter-clockwise in the flipped GL window; back faces and
    // degenerate triangles are not drawn.  Swapping vertices 1 and 2 makes the area positive for the edge functions.
    const double area = (T.u[1] - T.u[0]) * (T.v[2] - T.v[0]) - (T.u[2] - T.u[0]) * (T.v[1] - T.v[0]);
    if (!(area < 0.0)) return false;
    double t_;
    t_ = T.u[1]; T.u[1] = T.u[2]; T.u[2] = t_;
    t_ = T.v[1]; T.v[1] = T.v[2]; T.v[2] = t_;
    t_ = T.z[1]; T.z[1] = T.z[2]; T.z[2] = t_;
    T.A = -area;
    const double umin = fmin(T.u[0], fmin(T.u[1], T.u[2])), umax = fmax(T.u[0], fmax(T.u[1], T.u[2]));
    const double vmin = fmin(T.v[0], fmin(T.v[1], T.v[2])), vmax = fmax(T.v[0], fmax(T.v[1], T.v[2]));
    T.i0 = (int)fmax(0.0, ceil(umin - 0.5)); T.i1 = (int)fmin((double)(W - 1), floor(umax - 0.5));
    T.j0 = (int)fmax(0.0, ceil(vmin - 0.5)); T.j1 = (int)fmin((double)(H - 1), floor(vmax - 0.5));
    return T.i0 <= T.i1 && T.j0 <= T.j1;
}

// One pixel centre of a set-up triangle: coverage with the tie rule, 1/z interpolation, far clip, atomicMin on the float bits
// (Z = unsigned, the depth path) or on the winner key of triangle f (Z = WinnerKey, the colour path): one body, so both paths cover
// the same centres with the same depth.
template <typename Z>
__device__ __forceinline__ void tri_pixel(const TriSetup& T, int i, int j, Z* zrow_base, int W, int f)
{
    const double pu = i + 0.5, pv = j + 0.5;
    const double e0 = edge_fn(T.u[1], T.v[1], T.u[2], T.v[2], pu, pv);
    const double e1 = edge_fn(T.u[2], T.v[2], T.u[0], T.v[0], pu, pv);
    const double e2 = edge_fn(T.u[0], T.v[0], T.u[1], T.v[1], pu, pv);
    if (!(edge_in(e0, T.u[1], T.v[1], T.u[2], T.v[2]) && edge_in(e1, T.u[2], T.v[2], T.u[0], T.v[0]) &&
          edge_in(e2, T.u[0], T.v[0], T.u[1], T.v[1])))
        return;
    const double iz = (e0 / T.A) / T.z[0] + (e1 / T.A) / T.z[1] + (e2 / T.A) / T.z[2];
    const double d = 1.0 / iz;
    if (!(d >= CLIP_NEAR && d <= CLIP_FAR)) return;
    if constexpr (std::is_same<Z, WinnerKey>::value) atomicMin(zrow_base + (size_t)j * W + i, ((WinnerKey)__float_as_uint((float)d) << 32) | (unsigned)f);
    else atomicMin(zrow_base + (size_t)j * W + i, __float_as_uint((float)d));
}

// Route 1: one thread per triangle (blockIdx.y = job) walks its pixel box when the box holds at most BIG_TRI_PIXELS centres;
// larger triangles (near the camera, coarse meshes) are appended to `big` for route 2, so no thread walks a large box alone.
constexpr int BIG_TRI_PIXELS = 1024;
template <typename Z>
__global__ void __launch_bounds__(RASTER_THREADS) depth_raster_kernel(const RasterJob* __restrict__ jobs, Z* __restrict__ zbuf,
                                                                      int H, int W, int2* __restrict__ big, unsigned* __restrict__ n_big)
{
    const RasterJob& J = jobs[blockIdx.y];
    const int f = blockIdx.x * RASTER_THREADS + threadIdx.x;
    if (f >= J.n_tris) return;
    TriSetup T;
    if (!tri_setup(J, f, H, W, T)) return;
    if ((int64_t)(T.i1 - T.i0 + 1) * (T.j1 - T.j0 + 1) > BIG_TRI_PIXELS) {
        big[atomicAdd(n_big, 1u)] = make_int2((int)blockIdx.y, f);      // at most one entry per (job, triangle): within capacity
        return;
    }
    Z* zb = zbuf + (size_t)blockIdx.y * H * W;
    for (int j = T.j0; j <= T.j1; ++j)
        for (int i = T.i0; i <= T.i1; ++i) tri_pixel(T, i, j, zb, W, f);
}

// Route 2: one workgroup per large triangle, its threads striding over the pixel box.  The list order depends on scheduling;
// the result does not (atomicMin), so both routes together stay deterministic.
template <typename Z>
__global__ void __launch_bounds__(RASTER_THREADS) depth_raster_big_kernel(const RasterJob* __restrict__ jobs, Z* __restrict__ zbuf,
                                                                          int H, int W, const int2* __restrict__ big,
                                                                          const unsigned* __restrict__ n_big)
{
    const unsigned n = *n_big;
    for (unsigned e = blockIdx.x; e < n; e += gridDim.x) {
        const int2 jf = big[e];
        TriSetup T;
        if (!tri_setup(jobs[jf.x], jf.y, H, W, T)) continue;     // same set-up as route 1: succeeds
        Z* zb = zbuf + (size_t)jf.x * H * W;
        const int bw = T.i1 - T.i0 + 1;
        const int64_t npix = (int64_t)bw * (T.j1 - T.j0 + 1);
        for (int64_t q = threadIdx.x; q < npix; q += RASTER_THREADS) tri_pixel(T, T.i0 + (int)(q % bw), T.j0 + (int)(q / bw), zb, W, jf.y);
    }
}

__global__ void depth_finish_kernel(unsigned* __restrict__ zbuf, size_t n)
{
    for (size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x)
        if (zbuf[k] == DEPTH_EMPTY) zbuf[k] = 0u;        // +0.0f
}

// Colour path, after both raster routes: one thread per pixel of job blockIdx.y reads the winner key once, sets the winning triangle
// up again (the set-up of the raster routes: it succeeds and orders the vertices the same way) and evaluates the GL varying at the
// centre, perspective-correct: c = (sum b_i c_i / z_i) / (sum b_i / z_i) with the screen-space barycentrics b_i = e_i / A of the
// depth.  Nothing here depends on which route drew the triangle or on the order of the atomics.  The workgroup's 256 x 3 colour
// floats go through LDS so that consecutive threads store consecutive floats; the box of depth > 0 is reduced per wave, per
// workgroup, then with four atomics per workgroup that covers anything.
constexpr int RESOLVE_THREADS = 256;
__global__ void __launch_bounds__(RESOLVE_THREADS) xyz_resolve_kernel(const RasterJob* __restrict__ jobs, const WinnerKey* __restrict__ keys,
                                                                      int H, int W, float* __restrict__ color, float* __restrict__ depth,
                                                                      int* __restrict__ bbox)
{
    __shared__ float s_c[RESOLVE_THREADS * 3];
    __shared__ int s_bb[RESOLVE_THREADS / 64][4];
    const int job = blockIdx.y;
    const int HW = H * W;
    const int p0 = blockIdx.x * RESOLVE_THREADS;
    const int p = p0 + threadIdx.x;
    float c[3] = {0.f, 0.f, 0.f};
    float d = 0.f;
    int vlo = 0x7fffffff, ulo = 0x7fffffff, vhi = -1, uhi = -1;
    if (p < HW) {
        const WinnerKey key = keys[(size_t)job * HW + p];
        const RasterJob& J = jobs[job];
        const int f = (int)(unsigned)key;
        TriSetup T;
        // the set-up that drew the key succeeds again (same inputs, same code); were it not to, the pixel stays empty
        if (key != KEY_EMPTY && tri_setup(J, f, H, W, T)) {
            const int j = p / W, i = p - j * W;
            d = __uint_as_float((unsigned)(key >> 32));
            const double pu = i + 0.5, pv = j + 0.5;
            const double b0 = edge_fn(T.u[1], T.v[1], T.u[2], T.v[2], pu, pv) / T.A;
            const double b1 = edge_fn(T.u[2], T.v[2], T.u[0], T.v[0], pu, pv) / T.A;
            const double b2 = edge_fn(T.u[0], T.v[0], T.u[1], T.v[1], pu, pv) / T.A;
            const double iz = b0 / T.z[0] + b1 / T.z[1] + b2 / T.z[2];
            // tri_setup swapped vertices 1 and 2 for a positive area: the colours follow
            const float* c0 = J.colors + 3 * (size_t)J.tris[3 * (size_t)f];
            const float* c1 = J.colors + 3 * (size_t)J.tris[3 * (size_t)f + 2];
            const float* c2 = J.colors + 3 * (size_t)J.tris[3 * (size_t)f + 1];
            for (int k = 0; k < 3; ++k)
                c[k] = (float)(((b0 * (double)c0[k]) / T.z[0] + (b1 * (double)c1[k]) / T.z[1] + (b2 * (double)c2[k]) / T.z[2]) / iz);
            if (d > 0.f) { vlo = vhi = j; ulo = uhi = i; }
        }
        if (depth) depth[(size_t)job * HW + p] = d;
    }
    s_c[threadIdx.x * 3 + 0] = c[0]; s_c[threadIdx.x * 3 + 1] = c[1]; s_c[threadIdx.x * 3 + 2] = c[2];
    for (int o = 32; o > 0; o >>= 1) {
        vlo = min(vlo, __shfl_down(vlo, o, 64)); ulo = min(ulo, __shfl_down(ulo, o, 64));
        vhi = max(vhi, __shfl_down(vhi, o, 64)); uhi = max(uhi, __shfl_down(uhi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        int* b = s_bb[threadIdx.x >> 6];
        b[0] = vlo; b[1] = ulo; b[2] = vhi; b[3] = uhi;
    }
    __syncthreads();
    const int n_here = min(RESOLVE_THREADS, HW - p0) * 3;      // floats of this workgroup's pixels that exist
    float* out = color + ((size_t)job * HW + p0) * 3;
    for (int k = threadIdx.x; k < n_here; k += RESOLVE_THREADS) out[k] = s_c[k];
    if (threadIdx.x == 0) {
        for (int w = 1; w < RESOLVE_THREADS / 64; ++w) {
            vlo = min(vlo, s_bb[w][0]); ulo = min(ulo, s_bb[w][1]); vhi = max(vhi, s_bb[w][2]); uhi = max(uhi, s_bb[w][3]);
        }
        if (vhi >= 0) {
            atomicMin(bbox + 4 * job + 0, vlo); atomicMin(bbox + 4 * job + 1, ulo);
            atomicMax(bbox + 4 * job + 2, vhi); atomicMax(bbox + 4 * job + 3, uhi);
        }
    }
}

// bbox [n][4]: the neutral element before the resolve (FINISH = false), the [-1, -1, -1, -1] of an empty render after it
template <bool FINISH>
__global__ void xyz_bbox_kernel(int* __restrict__ bbox, int n_jobs)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_jobs) return;
    int* b = bbox + 4 * j;
    if (!FINISH) { b[0] = b[1] = 0x7fffffff; b[2] = b[3] = -1; }
    else if (b[2] < 0) b[0] = b[1] = -1;
}

// One workgroup per job.  Thread k takes pixels k, k + 256, ...; its partial sums are combined by a fixed tree, so the result of a
// job depends on nothing but its own inputs.
__global__ void __launch_bounds__(SCORE_THREADS) depth_score_kernel(const float* __restrict__ ref, const float* __restrict__ images,
                                                                    const int* __restrict__ img_of, const unsigned char* __restrict__ masks,
                                                                    int HW, unsigned char* __restrict__ inl_out,
                                                                    p2p_depth_score* __restrict__ out)
{
    __shared__ double s_fcn[SCORE_THREADS];
    __shared__ long long s_in[SCORE_THREADS], s_un[SCORE_THREADS];
    const int j = blockIdx.x;
    const float* dr = ref + (size_t)j * HW;
    const float* dt = images + (size_t)img_of[j] * HW;
    const unsigned char* m = masks + (size_t)j * HW;
    double fcn = 0.0;
    long long inl = 0, un = 0;
    for (int p = threadIdx.x; p < HW; p += SCORE_THREADS) {
        unsigned char keep = 0;
        if (m[p]) {
            ++un;
            const double diff = fabs((double)dr[p] - (double)dt[p]);
            if (diff < 0.02) { ++inl; keep = 1; }
            fcn += fmax(0.0, 0.02 - diff) / 0.02;
        }
        if (inl_out) inl_out[(size_t)j * HW + p] = keep;
    }
    s_fcn[threadIdx.x] = fcn; s_in[threadIdx.x] = inl; s_un[threadIdx.x] = un;
    __syncthreads();
    for (int w = SCORE_THREADS / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            s_fcn[threadIdx.x] += s_fcn[threadIdx.x + w];
            s_in[threadIdx.x] += s_in[threadIdx.x + w];
            s_un[threadIdx.x] += s_un[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[j].inlier_count = s_in[0];
        out[j].union_count = s_un[0];
        out[j].fcn = s_fcn[0];
        out[j].ratio = s_un[0] > 0 ? (double)s_in[0] / (double)s_un[0] : 0.0;
    }
}

}  // namespace

int check_jobs(const char* who, const p2p_mesh* const* meshes, int n_meshes, const p2p_refine_job* jobs, int n_jobs, int H, int W,
               int n_images)
{
    if (H <= 0 || W <= 0 || (int64_t)H * W > (1 << 26)) {
        set_error("%s: bad image size %d x %d", who, H, W);
        return P2P_ERR_INVALID_ARG;
    }
    for (int j = 0; j < n_jobs; ++j) {
        const p2p_refine_job& J = jobs[j];
        if (J.mesh_idx < 0 || J.mesh_idx >= n_meshes || !meshes[J.mesh_idx]) {
            set_error("%s: job %d names mesh %d of %d", who, j, J.mesh_idx, n_meshes);
            return P2P_ERR_INVALID_ARG;
        }
        if (n_images >= 0 && (J.img_idx < 0 || J.img_idx >= n_images || !J.union_mask)) {
            set_error("%s: job %d: image %d of %d, union_mask %p", who, j, J.img_idx, n_images, (const void*)J.union_mask);
            return P2P_ERR_INVALID_ARG;
        }
    }
    return P2P_OK;
}

namespace {

// Both raster routes of every job into zbuf [n_jobs][H][W] (device): float bits under DEPTH_EMPTY (Z = unsigned) or winner keys
// under KEY_EMPTY (Z = WinnerKey).  The job records stay at the front of djobs for the kernels that follow.
template <typename Z>
int raster_jobs(Ctx& X, const p2p_mesh* const* meshes, const p2p_refine_job* jobs, int n_jobs, int H, int W, Z* zbuf, DevBuf& djobs)
{
    hipStream_t st = X.stream;
    std::vector<RasterJob> rj(n_jobs);
    int max_tris = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const p2p_refine_job& J = jobs[j];
        const p2p_mesh* M = meshes[J.mesh_idx];
        if (M->device != X.device) {
            set_error("p2p depth: mesh %d lives on device %d, the context on device %d", J.mesh_idx, M->device, X.device);
            return P2P_ERR_INVALID_ARG;
        }
        RasterJob& r = rj[j];
        r.verts = M->verts; r.tris = M->tris; r.n_tris = M->n_tris; r.colors = M->colors;
        for (int k = 0; k < 9; ++k) r.R[k] = J.R[k];
        double tm[3];
        for (int k = 0; k < 3; ++k) tm[k] = J.t[k] / 1000.0;            // icp3d.py: render_obj(..., tra_pred/1000, ...)
        const bool quirk = tm[2] > 100.0;                               // render_obj: if(tra[2]>100): tra = tra/1000
        for (int k = 0; k < 3; ++k) r.t[k] = quirk ? tm[k] / 1000.0 : tm[k];
        r.fx = J.camK[0]; r.s = J.camK[1]; r.cx = J.camK[2]; r.fy = J.camK[4]; r.cy = J.camK[5];
        max_tris = std::max(max_tris, M->n_tris);
    }
    int rc;
    // job records, then the large-triangle counter and list (capacity: every (job, triangle) pair once)
    const size_t cap = (size_t)n_jobs * std::max(max_tris, 1);
    const size_t jb = (sizeof(RasterJob) * n_jobs + 255) / 256 * 256;
    if ((rc = djobs.reserve(jb + 256 + sizeof(int2) * cap))) return rc;
    RasterJob* dj = djobs.as<RasterJob>();
    unsigned* n_big = reinterpret_cast<unsigned*>(djobs.as<char>() + jb);
    int2* big = reinterpret_cast<int2*>(djobs.as<char>() + jb + 256);
    const size_t n = (size_t)n_jobs * H * W;
    HIP_TRY(hipMemcpyAsync(dj, rj.data(), sizeof(RasterJob) * n_jobs, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(n_big, 0, sizeof(unsigned), st));
    if constexpr (std::is_same<Z, WinnerKey>::value) HIP_TRY(hipMemsetAsync(zbuf, 0xff, n * sizeof(Z), st));      // KEY_EMPTY
    else HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)zbuf, (int)DEPTH_EMPTY, n, st));
    if (max_tris > 0) {
        dim3 grid((max_tris + RASTER_THREADS - 1) / RASTER_THREADS, n_jobs);
        depth_raster_kernel<Z><<<grid, RASTER_THREADS, 0, st>>>(dj, zbuf, H, W, big, n_big);
        HIP_TRY(hipGetLastError());
        depth_raster_big_kernel<Z><<<(unsigned)std::min<size_t>(cap, 1024), RASTER_THREADS, 0, st>>>(dj, zbuf, H, W, big, n_big);
        HIP_TRY(hipGetLastError());
    }
    return P2P_OK;
}

}  // namespace

// Renders every job into zbuf [n_jobs][H][W] (device, float bits), 0 where nothing is drawn.
int render_into(Ctx& X, const p2p_mesh* const* meshes, const p2p_refine_job* jobs, int n_jobs, int H, int W, unsigned* zbuf, DevBuf& djobs)
{
    int rc;
    if ((rc = raster_jobs(X, meshes, jobs, n_jobs, H, W, zbuf, djobs))) return rc;
    hipStream_t st = X.stream;
    const size_t n = (size_t)n_jobs * H * W;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 4096);
    depth_finish_kernel<<<blocks, 256, 0, st>>>(zbuf, n);
    HIP_TRY(hipGetLastError());
    return P2P_OK;
}

int score_into(Ctx& X, const p2p_mesh* const* meshes, const p2p_refine_job* jobs, int n_jobs, int H, int W, const float* images,
               const int* img_of, const unsigned char* masks, unsigned char* inl, p2p_depth_score* out, DevBuf& dz, DevBuf& djobs)
{
    const size_t HW = (size_t)H * W;
    int rc;
    if ((rc = dz.reserve(n_jobs * HW * 4)) || (rc = render_into(X, meshes, jobs, n_jobs, H, W, dz.as<unsigned>(), djobs))) return rc;
    depth_score_kernel<<<n_jobs, SCORE_THREADS, 0, X.stream>>>(dz.as<float>(), images, img_of, masks, (int)HW, inl, out);
    HIP_TRY(hipGetLastError());
    return P2P_OK;
}

}  // namespace p2p

using namespace p2p;

extern "C" {

int p2p_mesh_create(p2p_ctx* ctx, const float* verts_mm, int n_verts, const int* tris, int n_tris, p2p_mesh** out)
{
    if (!ctx || !out || n_verts <= 0 || n_tris < 0 || !verts_mm || (n_tris > 0 && !tris)) {
        set_error("p2p_mesh_create: bad arguments");
        return P2P_ERR_INVALID_ARG;
    }
    *out = nullptr;
    for (int64_t k = 0; k < 3 * (int64_t)n_tris; ++k)
        if (tris[k] < 0 || tris[k] >= n_verts) {
            set_error("p2p_mesh_create: triangle %lld names vertex %d of %d", (long long)(k / 3), tris[k], n_verts);
            return P2P_ERR_INVALID_ARG;
        }
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    HIP_TRY(hipSetDevice(c->device));
    std::vector<float> vm((size_t)n_verts * 3);
    for (size_t k = 0; k < vm.size(); ++k) vm[k] = verts_mm[k] * 0.001f;     // float32 x float32, as numpy scales a float32 cloud
    p2p_mesh* M = new p2p_mesh;
    M->device = c->device; M->n_verts = n_verts; M->n_tris = n_tris;
    hipError_t e = hipMalloc(&M->verts, vm.size() * 4);
    if (e == hipSuccess) e = hipMalloc(&M->tris, std::max<size_t>(1, (size_t)n_tris * 3) * 4);
    if (e == hipSuccess) e = hipMemcpy(M->verts, vm.data(), vm.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && n_tris > 0) e = hipMemcpy(M->tris, tris, (size_t)n_tris * 12, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_error("p2p_mesh_create: %s", hipGetErrorString(e));
        p2p_mesh_destroy(M);
        return P2P_ERR_HIP;
    }
    *out = M;
    return P2P_OK;
}

void p2p_mesh_destroy(p2p_mesh* mesh)
{
    if (!mesh) return;
    (void)hipSetDevice(mesh->device);
    if (mesh->verts) (void)hipFree(mesh->verts);
    if (mesh->tris) (void)hipFree(mesh->tris);
    if (mesh->colors) (void)hipFree(mesh->colors);
    delete mesh;
}

int p2p_render_depth_batch(p2p_ctx* ctx, const p2p_mesh* const* meshes, int n_meshes, const p2p_refine_job* jobs, int n_jobs, int height,
                           int width, float* depth)
{
    if (!ctx || n_jobs < 0 || (n_jobs > 0 && (!meshes || !jobs || !depth))) {
        set_error("p2p_render_depth_batch: bad arguments");
        return P2P_ERR_INVALID_ARG;
    }
    int rc;
    if ((rc = check_jobs("p2p_render_depth_batch", meshes, n_meshes, jobs, n_jobs, height, width, -1))) return rc;
    if (n_jobs == 0) return P2P_OK;
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)n_jobs * height * width;
    DevBuf dz, dj;
    if ((rc = dz.reserve(n * 4)) || (rc = render_into(*c, meshes, jobs, n_jobs, height, width, dz.as<unsigned>(), dj))) return rc;
    HIP_TRY(hipMemcpyAsync(depth, dz.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return P2P_OK;
}

int p2p_mesh_set_colors(p2p_mesh* mesh, const unsigned char* rgb, int n_verts)
{
    if (!mesh || !rgb) {
        set_error("p2p_mesh_set_colors: null %s", !mesh ? "mesh" : "colour array");
        return P2P_ERR_INVALID_ARG;
    }
    if (n_verts != mesh->n_verts) {
        set_error("p2p_mesh_set_colors: %d colours for a mesh of %d vertices", n_verts, mesh->n_verts);
        return P2P_ERR_INVALID_ARG;
    }
    // Replacing the colours of a mesh reuses its array.  Every render entry point synchronises its stream before it returns, so no
    // render of the calling thread is in flight here; a mesh shared with another thread's context must not be recoloured while that
    // thread renders it (a p2p_mesh is no more thread-safe than a p2p_ctx).
    HIP_TRY(hipSetDevice(mesh->device));
    std::vector<float> c((size_t)n_verts * 3);
    for (size_t k = 0; k < c.size(); ++k) c[k] = (float)rgb[k] / 255.0f;      // Model3D.load: float32 colours / 255
    if (!mesh->colors) HIP_TRY(hipMalloc(&mesh->colors, c.size() * 4));
    HIP_TRY(hipMemcpy(mesh->colors, c.data(), c.size() * 4, hipMemcpyHostToDevice));
    return P2P_OK;
}

int p2p_render_xyz_batch(p2p_ctx* ctx, const p2p_mesh* const* meshes, int n_meshes, const p2p_refine_job* jobs, int n_jobs, int height,
                         int width, float* color, float* depth, int* bbox)
{
    if (!ctx || n_jobs < 0 || (n_jobs > 0 && (!meshes || !jobs))) {
        set_error("p2p_render_xyz_batch: bad arguments");
        return P2P_ERR_INVALID_ARG;
    }
    if (n_jobs > 65535) {      // the raster and resolve grids carry the job in gridDim.y
        set_error("p2p_render_xyz_batch: %d jobs in one call, at most 65535", n_jobs);
        return P2P_ERR_INVALID_ARG;
    }
    if (n_jobs > 0 && !color) {
        set_error("p2p_render_xyz_batch: the colour buffer is null");
        return P2P_ERR_INVALID_ARG;
    }
    int rc;
    if ((rc = check_jobs("p2p_render_xyz_batch", meshes, n_meshes, jobs, n_jobs, height, width, -1))) return rc;
    for (int j = 0; j < n_jobs; ++j)
        if (!meshes[jobs[j].mesh_idx]->colors) {
            set_error("p2p_render_xyz_batch: job %d: mesh %d has no colours (p2p_mesh_set_colors)", j, jobs[j].mesh_idx);
            return P2P_ERR_INVALID_ARG;
        }
    if (n_jobs == 0) return P2P_OK;
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    HIP_TRY(hipSetDevice(c->device));
    if (!c->pipe) c->pipe = new Pipeline();
    Pipeline::XyzWork& Wk = c->pipe->xyz;
    hipStream_t st = c->stream;
    const size_t HW = (size_t)height * width, n = (size_t)n_jobs * HW;
    if ((rc = Wk.key.reserve(n * sizeof(WinnerKey))) || (rc = Wk.color.reserve(n * 12)) || (rc = Wk.depth.reserve(n * 4)) ||
        (rc = Wk.bbox.reserve(sizeof(int) * 4 * n_jobs)) ||
        (rc = raster_jobs(*c, meshes, jobs, n_jobs, height, width, Wk.key.as<WinnerKey>(), Wk.jobs)))
        return rc;
    const int bb_blocks = (n_jobs + 255) / 256;
    xyz_bbox_kernel<false><<<bb_blocks, 256, 0, st>>>(Wk.bbox.as<int>(), n_jobs);
    HIP_TRY(hipGetLastError());
    dim3 grid((unsigned)((HW + RESOLVE_THREADS - 1) / RESOLVE_THREADS), n_jobs);
    xyz_resolve_kernel<<<grid, RESOLVE_THREADS, 0, st>>>(Wk.jobs.as<RasterJob>(), Wk.key.as<WinnerKey>(), height, width, Wk.color.as<float>(),
                                                         Wk.depth.as<float>(), Wk.bbox.as<int>());
    HIP_TRY(hipGetLastError());
    xyz_bbox_kernel<true><<<bb_blocks, 256, 0, st>>>(Wk.bbox.as<int>(), n_jobs);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(color, Wk.color.p, n * 12, hipMemcpyDeviceToHost, st));
    if (depth) HIP_TRY(hipMemcpyAsync(depth, Wk.depth.p, n * 4, hipMemcpyDeviceToHost, st));
    if (bbox) HIP_TRY(hipMemcpyAsync(bbox, Wk.bbox.p, sizeof(int) * 4 * n_jobs, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return P2P_OK;
}

int p2p_depth_score_batch(p2p_ctx* ctx, const p2p_mesh* const* meshes, int n_meshes, const float* const* depth_images, int n_images,
                          const p2p_refine_job* jobs, int n_jobs, int height, int width, p2p_depth_score* out, unsigned char* inlier_masks)
{
    if (!ctx || n_jobs < 0 || n_images < 0 || (n_jobs > 0 && (!meshes || !jobs || !out || !depth_images))) {
        set_error("p2p_depth_score_batch: bad arguments");
        return P2P_ERR_INVALID_ARG;
    }
    int rc;
    if ((rc = check_jobs("p2p_depth_score_batch", meshes, n_meshes, jobs, n_jobs, height, width, n_images))) return rc;
    for (int i = 0; i < n_images; ++i)
        if (!depth_images[i]) {
            set_error("p2p_depth_score_batch: depth image %d is null", i);
            return P2P_ERR_INVALID_ARG;
        }
    if (n_jobs == 0) return P2P_OK;
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t HW = (size_t)height * width;
    DevBuf dz, dj, dimg, dmask, dof, dinl, dout;
    if ((rc = dimg.reserve(n_images * HW * 4)) || (rc = dmask.reserve(n_jobs * HW)) ||
        (rc = dof.reserve(sizeof(int) * n_jobs)) || (rc = dout.reserve(sizeof(p2p_depth_score) * n_jobs)) ||
        (inlier_masks && (rc = dinl.reserve(n_jobs * HW))))
        return rc;
    std::vector<int> img_of(n_jobs);
    for (int j = 0; j < n_jobs; ++j) img_of[j] = jobs[j].img_idx;
    for (int i = 0; i < n_images; ++i)
        HIP_TRY(hipMemcpyAsync(dimg.as<float>() + i * HW, depth_images[i], HW * 4, hipMemcpyHostToDevice, st));
    for (int j = 0; j < n_jobs; ++j)
        HIP_TRY(hipMemcpyAsync(dmask.as<unsigned char>() + j * HW, jobs[j].union_mask, HW, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dof.p, img_of.data(), sizeof(int) * n_jobs, hipMemcpyHostToDevice, st));
    if ((rc = score_into(*c, meshes, jobs, n_jobs, height, width, dimg.as<float>(), dof.as<int>(), dmask.as<unsigned char>(),
                         inlier_masks ? dinl.as<unsigned char>() : nullptr, dout.as<p2p_depth_score>(), dz, dj)))
        return rc;
    HIP_TRY(hipMemcpyAsync(out, dout.p, sizeof(p2p_depth_score) * n_jobs, hipMemcpyDeviceToHost, st));
    if (inlier_masks) HIP_TRY(hipMemcpyAsync(inlier_masks, dinl.p, n_jobs * HW, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return P2P_OK;
}

}  // extern "C"
