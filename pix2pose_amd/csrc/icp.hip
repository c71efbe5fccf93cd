// Point-to-plane ICP (a named restatement of cv::ppf_match_3d::ICP::registerModelToScene, opencv-contrib 3.4.2) and the depth
// refinement entry point (reference tools/5_evaluation_bop_icp3d.py icp_refinement :86-94 and the score at :466-491).  The rules
// (normalisation, pyramid, float32 nearest neighbour and its tie rule, the lower medians of the rejection, the picky selection, the
// float64 point-to-plane solve, getTransformMat) are written down in DESIGN.md section 8.2; tests/icp_ref.py restates them in numpy.
//
// Every job of a call iterates together and its loop state lives on the device (IcpJob): a job that has converged or broken is
// inactive and every later launch returns at once for it.  All reductions use fixed partitions and a fixed tree (integer atomics
// only count, or pick by a key whose minimum does not depend on order), so a job's result does not depend on the rest of the batch.
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

constexpr int PT_THREADS = 256;        // per-point kernels
constexpr int JOB_THREADS = 256;       // one workgroup per job
constexpr int CHECK_EVERY = 4;         // iterations queued between two reads of the active-job count (measured)
constexpr double FVAL_INIT = 9999999999.0;
constexpr double NORMAL_EPS = 2.22e-16;
constexpr double EIG_REL = 1e-12;      // eigenvalues of A^T A below EIG_REL * the largest are taken as 0 (singular values < 1e-6 sigma_max)
constexpr unsigned long long NO_KEY = ~0ull;

struct IcpLevel {
    int np, nq, step, max_it;          // |P|, |Q|, sampling step, rint(I / (l + 1))
    double tolp;                       // tolerance * (l + 1)^2
};

struct IcpJob {
    int64_t soff, toff;                // first point of the job in the source (S0, P, M, ...) and target (T0, Q, ...) arrays
    int64_t in_s, in_t;                // first point of the job in the caller's source and target arrays (p2p_icp_input offsets)
    int64_t coff;                      // first entry of the job's cell arrays (toff + 2 * job)
    int n, m;
    int status;
    int level;                         // index into the per-level results (0 = finest)
    int active, it, pairs;
    int np, nq, step, max_it;
    double tolp;
    float thr;
    int keep_all;                      // rejection_scale <= 0
    double fval_old, fval_perc, fval_min;
    double X[16], pose[16];
    double mean_avg[3], scale;
    double lo[3], h;                   // the level's grid over Q
    int dims[3], ncells;
    int iterations[P2P_ICP_MAX_LEVELS], pairs_lv[P2P_ICP_MAX_LEVELS];
    double fval_min_lv[P2P_ICP_MAX_LEVELS];
};

// -------------------------------------------------------------------------------------------------------------------------------------
// Normalisation

// One wave per job: lanes 0 and 1 sum the source / target xyz sequentially in float64 (the restatement's np.cumsum order), check them
// for non-finite values, then sum the distances to the origin of the centred float32 points the same way.
__global__ void __launch_bounds__(64) icp_stats_kernel(IcpJob* __restrict__ jobs, const float* __restrict__ S, const float* __restrict__ T)
{
    IcpJob& J = jobs[blockIdx.x];
    __shared__ double s_mean[2][3];
    __shared__ int s_bad[2];
    __shared__ double s_dist[2];
    const int lane = threadIdx.x;
    if (J.status != 0) return;
    if (lane < 2) {
        const float* A = lane == 0 ? S + J.in_s * 6 : T + J.in_t * 6;
        const int n = lane == 0 ? J.n : J.m;
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int bad = 0;
        for (int i = 0; i < n; ++i) {
            const float x = A[(size_t)i * 6], y = A[(size_t)i * 6 + 1], z = A[(size_t)i * 6 + 2];
            bad |= !(isfinite(x) && isfinite(y) && isfinite(z));
            sx += (double)x; sy += (double)y; sz += (double)z;
        }
        s_mean[lane][0] = sx / (double)n; s_mean[lane][1] = sy / (double)n; s_mean[lane][2] = sz / (double)n;
        s_bad[lane] = bad;
    }
    __syncthreads();
    if (s_bad[0] | s_bad[1]) {
        if (lane == 0) J.status = P2P_ICP_NONFINITE;
        return;
    }
    double ma[3];
    for (int q = 0; q < 3; ++q) ma[q] = 0.5 * (s_mean[0][q] + s_mean[1][q]);
    if (lane < 2) {
        const float* A = lane == 0 ? S + J.in_s * 6 : T + J.in_t * 6;
        const int n = lane == 0 ? J.n : J.m;
        const float mx = (float)ma[0], my = (float)ma[1], mz = (float)ma[2];
        double d = 0.0;
        for (int i = 0; i < n; ++i) {
            const double x = (double)(A[(size_t)i * 6] - mx), y = (double)(A[(size_t)i * 6 + 1] - my), z = (double)(A[(size_t)i * 6 + 2] - mz);
            d += sqrt((x * x + y * y) + z * z);
        }
        s_dist[lane] = d;
    }
    __syncthreads();
    if (lane == 0) {
        for (int q = 0; q < 3; ++q) J.mean_avg[q] = ma[q];
        J.scale = (double)J.n / ((s_dist[0] + s_dist[1]) * 0.5);
        for (int k = 0; k < 16; ++k) J.pose[k] = (k % 5 == 0) ? 1.0 : 0.0;
        // every point at the mean (zero distance sum) or a float32 overflow: no finite normalisation
        const double sf = (double)(float)J.scale;
        if (!(isfinite(sf) && sf > 0.0)) J.status = P2P_ICP_NONFINITE;
    }
}

// S0 / T0: xyz - float32(meanAvg), then * float32(scale), both in float32; normals as they are.  blockIdx.z: 0 source, 1 target.
__global__ void __launch_bounds__(PT_THREADS) icp_normalise_kernel(const IcpJob* __restrict__ jobs, const float* __restrict__ S,
                                                                   const float* __restrict__ T, float* __restrict__ S0, float* __restrict__ T0)
{
    const IcpJob& J = jobs[blockIdx.y];
    const int i = blockIdx.x * PT_THREADS + threadIdx.x;
    if (J.status != 0 || i >= (blockIdx.z ? J.m : J.n)) return;
    const float* a = (blockIdx.z ? T + (J.in_t + i) * 6 : S + (J.in_s + i) * 6);
    float* b = (blockIdx.z ? T0 + (J.toff + i) * 6 : S0 + (J.soff + i) * 6);
    const float sc = (float)J.scale;
    for (int q = 0; q < 3; ++q) b[q] = (a[q] - (float)J.mean_avg[q]) * sc;
    for (int q = 3; q < 6; ++q) b[q] = a[q];
}

// -------------------------------------------------------------------------------------------------------------------------------------
// Levels

// transformPCPose: xyz = float32(R p + t) in float64, normal = float32(R n / |R n|) (left 0 when |R n| <= 2.22e-16)
__device__ __forceinline__ void transform_pt(const double* X, const float* a, float* b, bool normals)
{
    const double x = a[0], y = a[1], z = a[2];
    for (int r = 0; r < 3; ++r) b[r] = (float)(((X[4 * r] * x + X[4 * r + 1] * y) + X[4 * r + 2] * z) + X[4 * r + 3]);
    if (!normals) return;
    const double nx = a[3], ny = a[4], nz = a[5];
    double n2[3];
    for (int r = 0; r < 3; ++r) n2[r] = (X[4 * r] * nx + X[4 * r + 1] * ny) + X[4 * r + 2] * nz;
    const double nn = sqrt((n2[0] * n2[0] + n2[1] * n2[1]) + n2[2] * n2[2]);
    for (int r = 0; r < 3; ++r) b[3 + r] = nn > NORMAL_EPS ? (float)(n2[r] / nn) : 0.0f;
}

__global__ void icp_level_kernel(IcpJob* __restrict__ jobs, int n_jobs, const IcpLevel* __restrict__ lv, int level)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_jobs) return;
    IcpJob& J = jobs[j];
    J.level = level;
    J.active = 0;
    if (J.status != 0) return;
    const IcpLevel& L = lv[j];
    J.np = L.np; J.nq = L.nq; J.step = L.step; J.max_it = L.max_it; J.tolp = L.tolp;
    for (int k = 0; k < 16; ++k) J.X[k] = (k % 5 == 0) ? 1.0 : 0.0;
    J.fval_old = FVAL_INIT; J.fval_min = FVAL_INIT; J.fval_perc = 0.0;
    J.it = 0; J.pairs = 0;
    const bool conv = J.fval_perc < 1.0 + J.tolp && J.fval_perc > 1.0 - J.tolp;
    J.active = J.nq > 0 && !conv && J.it < J.max_it;
}

// P = transform(S0, pose) at rows 0, step, 2 step, ...; M = P's xyz; Q = T0 at the same step (blockIdx.z 0: P, 1: Q).
__global__ void __launch_bounds__(PT_THREADS) icp_sample_kernel(const IcpJob* __restrict__ jobs, const float* __restrict__ S0,
                                                                const float* __restrict__ T0, float* __restrict__ P, float4* __restrict__ M,
                                                                float* __restrict__ Q)
{
    const IcpJob& J = jobs[blockIdx.y];
    const int k = blockIdx.x * PT_THREADS + threadIdx.x;
    if (!J.active) return;
    if (blockIdx.z == 0) {
        if (k >= J.np) return;
        float* p = P + (J.soff + k) * 6;
        transform_pt(J.pose, S0 + (J.soff + (int64_t)k * J.step) * 6, p, true);
        M[J.soff + k] = make_float4(p[0], p[1], p[2], 0.0f);
    } else {
        if (k >= J.nq) return;
        const float* a = T0 + (J.toff + (int64_t)k * J.step) * 6;
        float* q = Q + (J.toff + k) * 6;
        for (int c = 0; c < 6; ++c) q[c] = a[c];
    }
}

// After a level: pose = X * pose, and the level's counts.
__global__ void icp_level_end_kernel(IcpJob* __restrict__ jobs, int n_jobs)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_jobs) return;
    IcpJob& J = jobs[j];
    if (J.status != 0) return;
    double r[16];
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) {
            double s = J.X[4 * a] * J.pose[b];
            for (int k = 1; k < 4; ++k) s = s + J.X[4 * a + k] * J.pose[4 * k + b];
            r[4 * a + b] = s;
        }
    for (int k = 0; k < 16; ++k) J.pose[k] = r[k];
    J.iterations[J.level] = J.it;
    J.pairs_lv[J.level] = J.pairs;
    J.fval_min_lv[J.level] = J.fval_min;
    J.active = 0;
}

// Undo the normalisation: t' = t / scale + meanAvg - R meanAvg.
__global__ void icp_finish_kernel(IcpJob* __restrict__ jobs, int n_jobs)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_jobs) return;
    IcpJob& J = jobs[j];
    if (J.status != 0) return;
    for (int r = 0; r < 3; ++r) {
        const double rm = (J.pose[4 * r] * J.mean_avg[0] + J.pose[4 * r + 1] * J.mean_avg[1]) + J.pose[4 * r + 2] * J.mean_avg[2];
        J.pose[4 * r + 3] = (J.pose[4 * r + 3] / J.scale + J.mean_avg[r]) - rm;
    }
}

// -------------------------------------------------------------------------------------------------------------------------------------
// Uniform grid over a level's Q: cubic cells of side h, at most max(|Q|, 1) cells.  Points are bucketed by a counting sort; the order
// inside a cell depends on scheduling, the search does not (it keeps the least (d2, j)).

__device__ __forceinline__ int cell_axis(double v, double lo, double h, int dim)
{
    const double f = floor((v - lo) / h);
    return !(f >= 0.0) ? 0 : (f >= (double)(dim - 1) ? dim - 1 : (int)f);        // (NaN -> 0: every index stays in the grid)
}

__device__ double grid_cells(const double* e, double h)
{
    double c = 1.0;
    for (int a = 0; a < 3; ++a) c *= fmin(floor(e[a] / h), 1e9) + 1.0;
    return c;
}

__global__ void __launch_bounds__(JOB_THREADS) icp_grid_bbox_kernel(IcpJob* __restrict__ jobs, const float* __restrict__ Q,
                                                                    int* __restrict__ cnt)
{
    IcpJob& J = jobs[blockIdx.x];
    if (!J.active) return;
    __shared__ float s_lo[3][JOB_THREADS], s_hi[3][JOB_THREADS];
    __shared__ int s_n;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = threadIdx.x; k < J.nq; k += JOB_THREADS)
        for (int a = 0; a < 3; ++a) {
            const float v = Q[(J.toff + k) * 6 + a];
            lo[a] = fminf(lo[a], v); hi[a] = fmaxf(hi[a], v);
        }
    for (int a = 0; a < 3; ++a) { s_lo[a][threadIdx.x] = lo[a]; s_hi[a][threadIdx.x] = hi[a]; }
    __syncthreads();
    for (int w = JOB_THREADS / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w)
            for (int a = 0; a < 3; ++a) {
                s_lo[a][threadIdx.x] = fminf(s_lo[a][threadIdx.x], s_lo[a][threadIdx.x + w]);
                s_hi[a][threadIdx.x] = fmaxf(s_hi[a][threadIdx.x], s_hi[a][threadIdx.x + w]);
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double e[3], emax = 0.0;
        for (int a = 0; a < 3; ++a) {
            J.lo[a] = s_lo[a][0];
            e[a] = (double)s_hi[a][0] - (double)s_lo[a][0];
            emax = fmax(emax, e[a]);
        }
        const double target = (double)max(J.nq, 1);
        double h;
        if (!(emax > 0.0)) {
            h = 1.0;
        } else {
            // least h (to bisection precision) with at most `target` cells: grid_cells is non-increasing in h
            double hl = emax / (target + 1.0), hh = emax * 1.0000001;     // cells(hl) > target >= cells(hh) = 1
            for (int it = 0; it < 60; ++it) {
                const double hm = 0.5 * (hl + hh);
                if (grid_cells(e, hm) <= target) hh = hm; else hl = hm;
            }
            h = hh;
        }
        if (!(isfinite(h) && h > 0.0 && isfinite(emax))) {    // (cannot happen for finite points; keeps the grid in bounds)
            h = 1.0;
            e[0] = e[1] = e[2] = 0.0;
        }
        J.h = h;
        int nc = 1;
        for (int a = 0; a < 3; ++a) {
            const double d = floor(e[a] / h);
            J.dims[a] = (d >= 0.0 && d < target) ? (int)d + 1 : (d >= target ? (int)target : 1);
            nc *= J.dims[a];
        }
        if (nc > (int)target) {
            J.dims[0] = J.dims[1] = J.dims[2] = 1;
            nc = 1;
        }
        J.ncells = nc;
        s_n = nc;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < s_n; c += JOB_THREADS) cnt[J.coff + c] = 0;
}

__global__ void __launch_bounds__(PT_THREADS) icp_grid_count_kernel(const IcpJob* __restrict__ jobs, const float* __restrict__ Q,
                                                                    int* __restrict__ qcell, int* __restrict__ cnt)
{
    const IcpJob& J = jobs[blockIdx.y];
    const int k = blockIdx.x * PT_THREADS + threadIdx.x;
    if (!J.active || k >= J.nq) return;
    const float* q = Q + (J.toff + k) * 6;
    const int cx = cell_axis(q[0], J.lo[0], J.h, J.dims[0]), cy = cell_axis(q[1], J.lo[1], J.h, J.dims[1]),
              cz = cell_axis(q[2], J.lo[2], J.h, J.dims[2]);
    const int c = (cz * J.dims[1] + cy) * J.dims[0] + cx;
    qcell[J.toff + k] = c;
    atomicAdd(cnt + J.coff + c, 1);
}

// Exclusive scan of the cell counts into start (ncells + 1 entries) and the write cursors.
__global__ void __launch_bounds__(JOB_THREADS) icp_grid_scan_kernel(const IcpJob* __restrict__ jobs, const int* __restrict__ cnt,
                                                                    int* __restrict__ start, int* __restrict__ cursor)
{
    const IcpJob& J = jobs[blockIdx.x];
    if (!J.active) return;
    __shared__ int s[JOB_THREADS];
    const int nc = J.ncells, per = (nc + JOB_THREADS - 1) / JOB_THREADS;
    const int c0 = min(nc, (int)threadIdx.x * per), c1 = min(nc, c0 + per);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += cnt[J.coff + c];
    s[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < JOB_THREADS; ++t) { const int v = s[t]; s[t] = run; run += v; }
    }
    __syncthreads();
    int run = s[threadIdx.x];
    for (int c = c0; c < c1; ++c) {
        start[J.coff + c] = run;
        cursor[J.coff + c] = run;
        run += cnt[J.coff + c];
    }
    if (threadIdx.x == 0) start[J.coff + nc] = J.nq;
}

__global__ void __launch_bounds__(PT_THREADS) icp_grid_scatter_kernel(const IcpJob* __restrict__ jobs, const float* __restrict__ Q,
                                                                      const int* __restrict__ qcell, int* __restrict__ cursor,
                                                                      float4* __restrict__ qs)
{
    const IcpJob& J = jobs[blockIdx.y];
    const int k = blockIdx.x * PT_THREADS + threadIdx.x;
    if (!J.active || k >= J.nq) return;
    const float* q = Q + (J.toff + k) * 6;
    const int at = atomicAdd(cursor + J.coff + qcell[J.toff + k], 1);
    qs[J.toff + at] = make_float4(q[0], q[1], q[2], __int_as_float(k));
}

// -------------------------------------------------------------------------------------------------------------------------------------
// One iteration: nearest neighbour, rejection, picky selection, solve, move.

// d2 = float32((dx dx + dy dy) + dz dz), dx = M.x - Q.x in float32; the least (d2, j) wins (ties to the lowest j).
__device__ __forceinline__ void nn_try(float mx, float my, float mz, float4 q, int j, float& best, int& bj)
{
    const float dx = mx - q.x, dy = my - q.y, dz = mz - q.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2 < best || (d2 == best && j < bj)) { best = d2; bj = j; }
}

// Grid route: rings of cells around the query's cell (Chebyshev radius r = 0, 1, ...) until the distance from the query to every cell
// outside the searched block exceeds the best d2 with a margin that covers float32 rounding of d2 and float64 rounding of the cell
// edges.  Every point that could tie or beat the best is visited, so the answer equals the brute-force scan, ties included.
__global__ void __launch_bounds__(PT_THREADS) icp_nn_grid_kernel(const IcpJob* __restrict__ jobs, const float4* __restrict__ M,
                                                                 const float4* __restrict__ qs, const int* __restrict__ start,
                                                                 int* __restrict__ jidx, float* __restrict__ d2out)
{
    const IcpJob& J = jobs[blockIdx.y];
    const int i = blockIdx.x * PT_THREADS + threadIdx.x;
    if (!J.active || i >= J.np) return;
    const float4 m = M[J.soff + i];
    const double p[3] = {m.x, m.y, m.z};
    int c[3];
    for (int a = 0; a < 3; ++a) c[a] = cell_axis(p[a], J.lo[a], J.h, J.dims[a]);
    const int* st = start + J.coff;
    const float4* Qs = qs + J.toff;
    float best = INFINITY;
    int bj = 0;                 // the lowest row: also the answer when every d2 is +inf
    const int rmax = max(J.dims[0], max(J.dims[1], J.dims[2]));
    for (int r = 0; r <= rmax; ++r) {
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, J.dims[2] - 1);
        const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, J.dims[1] - 1);
        const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, J.dims[0] - 1);
        auto visit = [&](int x, int y, int z) {
            const int cell = (z * J.dims[1] + y) * J.dims[0] + x;
            for (int e = st[cell]; e < st[cell + 1]; ++e) {
                const float4 q = Qs[e];
                nn_try(m.x, m.y, m.z, q, __float_as_int(q.w), best, bj);
            }
        };
        for (int z = z0; z <= z1; ++z)
            for (int y = y0; y <= y1; ++y) {
                if (abs(z - c[2]) == r || abs(y - c[1]) == r) {        // a face row of the shell: every cell of the row
                    for (int x = x0; x <= x1; ++x) visit(x, y, z);
                } else {                                                // inside: the two end cells (r > 0 here)
                    if (c[0] - r >= 0) visit(c[0] - r, y, z);
                    if (c[0] + r < J.dims[0]) visit(c[0] + r, y, z);
                }
            }
        // lower bound of the distance to any cell outside the block of radius r (only sides where cells remain)
        double lb = INFINITY;
        for (int a = 0; a < 3; ++a) {
            if (c[a] - r > 0) lb = fmin(lb, p[a] - (J.lo[a] + (double)(c[a] - r) * J.h));
            if (c[a] + r < J.dims[a] - 1) lb = fmin(lb, (J.lo[a] + (double)(c[a] + r + 1) * J.h) - p[a]);
        }
        if (lb == INFINITY) break;                                   // the block covers the grid
        lb -= 1e-6 * J.h;
        if (lb > 0.0 && lb * lb > (double)best * (1.0 + 1e-5)) break;
    }
    jidx[J.soff + i] = bj;
    d2out[J.soff + i] = best;
}

// Brute-force route (development twin, P2P_ICP_BRUTE=1): every Q row, in tiles of PT_THREADS rows staged in LDS, in index order.
__global__ void __launch_bounds__(PT_THREADS) icp_nn_brute_kernel(const IcpJob* __restrict__ jobs, const float4* __restrict__ M,
                                                                  const float* __restrict__ Q, int* __restrict__ jidx,
                                                                  float* __restrict__ d2out)
{
    const IcpJob& J = jobs[blockIdx.y];
    if (!J.active) return;                                           // uniform over the workgroup
    const int i = blockIdx.x * PT_THREADS + threadIdx.x;
    if ((int)(blockIdx.x * PT_THREADS) >= J.np) return;              // uniform too
    __shared__ float4 tile[PT_THREADS];
    const float4 m = i < J.np ? M[J.soff + i] : make_float4(0.f, 0.f, 0.f, 0.f);
    float best = INFINITY;
    int bj = 0;                 // the lowest row: also the answer when every d2 is +inf
    for (int t0 = 0; t0 < J.nq; t0 += PT_THREADS) {
        const int k = t0 + threadIdx.x;
        if (k < J.nq) {
            const float* q = Q + (J.toff + k) * 6;
            tile[threadIdx.x] = make_float4(q[0], q[1], q[2], 0.0f);
        }
        __syncthreads();
        const int nt = min(PT_THREADS, J.nq - t0);
        for (int e = 0; e < nt; ++e) nn_try(m.x, m.y, m.z, tile[e], t0 + e, best, bj);
        __syncthreads();
    }
    if (i < J.np) {
        jidx[J.soff + i] = bj;
        d2out[J.soff + i] = best;
    }
}

// k-th smallest (0-based) of n non-negative float32 values by a radix select on their bits (non-negative floats order as their bits);
// DEV: the values are float32(|double(d2) - double(med)|).  All threads of the workgroup call it.
template <bool DEV>
__device__ unsigned block_select(const float* __restrict__ v, int n, int k, float med)
{
    __shared__ int hist[256];
    __shared__ int s_sel, s_k;
    unsigned prefix = 0, mask = 0;
    if (threadIdx.x == 0) s_k = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int b = threadIdx.x; b < 256; b += JOB_THREADS) hist[b] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += JOB_THREADS) {
            const float x = DEV ? (float)fabs((double)v[i] - (double)med) : v[i];
            const unsigned b = __float_as_uint(x);
            if ((b & mask) == prefix) atomicAdd(&hist[(b >> shift) & 255u], 1);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int acc = 0, sel = 255;
            for (int d = 0; d < 256; ++d) {
                if (s_k < acc + hist[d]) { sel = d; break; }
                acc += hist[d];
            }
            s_k -= acc;
            s_sel = sel;
        }
        __syncthreads();
        prefix |= (unsigned)s_sel << shift;
        mask |= 255u << shift;
        __syncthreads();
    }
    return prefix;
}

// Robust rejection: thr = rho * 1.48257968 * lowermedian(|d2 - med|) + med, med = lowermedian(d2) (float32, no FMA); clears the keys.
__global__ void __launch_bounds__(JOB_THREADS) icp_select_kernel(IcpJob* __restrict__ jobs, const float* __restrict__ d2,
                                                                 unsigned long long* __restrict__ keys, float rho)
{
    IcpJob& J = jobs[blockIdx.x];
    if (!J.active) return;
    for (int k = threadIdx.x; k < J.nq; k += JOB_THREADS) keys[J.toff + k] = NO_KEY;
    if (J.keep_all) return;
    const float* v = d2 + J.soff;
    const int kk = (J.np - 1) / 2;
    const float med = __uint_as_float(block_select<false>(v, J.np, kk, 0.0f));
    const float mdev = __uint_as_float(block_select<true>(v, J.np, kk, med));
    if (threadIdx.x == 0) {
        const float s = 1.48257968f * mdev;
        const float t = rho * s;
        J.thr = t + med;
    }
}

// Picky ICP: per target row the least (d2, then highest i) kept pair, as one uint64 key reduced with atomicMin.
__global__ void __launch_bounds__(PT_THREADS) icp_picky_kernel(const IcpJob* __restrict__ jobs, const int* __restrict__ jidx,
                                                               const float* __restrict__ d2, unsigned long long* __restrict__ keys)
{
    const IcpJob& J = jobs[blockIdx.y];
    const int i = blockIdx.x * PT_THREADS + threadIdx.x;
    if (!J.active || i >= J.np) return;
    const float d = d2[J.soff + i];
    if (!J.keep_all && !(d < J.thr)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
    atomicMin(keys + J.toff + jidx[J.soff + i], key);
}

constexpr int NSUM = 21 + 6 + 1 + 1;    // A^T A (upper triangle), A^T b, fval sum, selInd

// Jacobi eigen-decomposition of the symmetric 6 x 6 a (destroyed: eigenvalues on its diagonal, eigenvectors in the columns of v).
// Cyclic sweeps; an off-diagonal entry below 1e-18 (|a_pp| + |a_qq|) is set to 0 without a rotation; stops after a sweep without a
// rotation (at most 50 sweeps).  tests/icp_ref.py runs the same loop.
__device__ __host__ inline void jacobi6(double a[6][6], double v[6][6])
{
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) v[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 50; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 5; ++p)
            for (int q = p + 1; q < 6; ++q) {
                const double apq = a[p][q];
                if (fabs(apq) <= 1e-18 * (fabs(a[p][p]) + fabs(a[q][q]))) {
                    a[p][q] = 0.0; a[q][p] = 0.0;
                    continue;
                }
                rotated = true;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 6; ++k) {
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq;
                    a[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 6; ++k) {
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk;
                    a[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 6; ++k) {
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq;
                    v[k][q] = s * vkp + c * vkq;
                }
            }
        if (!rotated) break;
    }
}

// Sums of the selected pairs (thread t takes target rows t, t + 256, ...; a fixed butterfly within each wave, then the waves in order),
// then on thread 0: the break at selInd < 6, the minimum-norm solve, X = getTransformMat(x), fval and the loop condition.
__global__ void __launch_bounds__(JOB_THREADS) icp_solve_kernel(IcpJob* __restrict__ jobs, const float* __restrict__ P,
                                                                const float* __restrict__ Q, const unsigned long long* __restrict__ keys,
                                                                int* __restrict__ n_active)
{
    IcpJob& J = jobs[blockIdx.x];
    if (!J.active) return;
    double acc[NSUM];
    for (int k = 0; k < NSUM; ++k) acc[k] = 0.0;
    for (int j = threadIdx.x; j < J.nq; j += JOB_THREADS) {
        const unsigned long long key = keys[J.toff + j];
        if (key == NO_KEY) continue;
        const int i = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
        const float* pf = P + (J.soff + i) * 6;
        const float* qf = Q + (J.toff + j) * 6;
        const double p0 = pf[0], p1 = pf[1], p2 = pf[2], q0 = qf[0], q1 = qf[1], q2 = qf[2], n0 = qf[3], n1 = qf[4], n2 = qf[5];
        const double a[6] = {p1 * n2 - p2 * n1, p2 * n0 - p0 * n2, p0 * n1 - p1 * n0, n0, n1, n2};
        const double b = ((q0 - p0) * n0 + (q1 - p1) * n1) + (q2 - p2) * n2;
        int e = 0;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c) acc[e++] += a[r] * a[c];
        for (int r = 0; r < 6; ++r) acc[21 + r] += a[r] * b;
        double f = 0.0;
        for (int c = 0; c < 6; ++c) {
            const double d = (double)pf[c] - (double)qf[c];
            f += d * d;
        }
        acc[27] += f;
        acc[28] += 1.0;
    }
    for (int w = 32; w > 0; w >>= 1)
        for (int k = 0; k < NSUM; ++k) acc[k] += __shfl_xor(acc[k], w);
    __shared__ double s_acc[JOB_THREADS / 64][NSUM];
    const int wave = threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < NSUM; ++k) s_acc[wave][k] = acc[k];
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 0; k < NSUM; ++k) {
        double s = s_acc[0][k];
        for (int w = 1; w < JOB_THREADS / 64; ++w) s += s_acc[w][k];
        acc[k] = s;
    }
    const int sel = (int)acc[28];
    J.pairs = sel;
    bool go = false;
    if (sel >= 6) {
        double ata[6][6], v[6][6];
        int e = 0;
        for (int r = 0; r < 6; ++r)
            for (int c = r; c < 6; ++c) { ata[r][c] = acc[e]; ata[c][r] = acc[e]; ++e; }
        jacobi6(ata, v);
        double lmax = 0.0;
        for (int r = 0; r < 6; ++r) lmax = fmax(lmax, ata[r][r]);
        double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < 6; ++k) {
            const double l = ata[k][k];
            if (!(l > EIG_REL * lmax)) continue;
            double d = 0.0;
            for (int r = 0; r < 6; ++r) d += v[r][k] * acc[21 + r];
            const double cf = d / l;
            for (int r = 0; r < 6; ++r) x[r] += cf * v[r][k];
        }
        bool nan = false;
        for (int r = 0; r < 6; ++r) nan |= isnan(x[r]);
        if (!nan) {
            // getTransformMat: Rz(x2) Ry(x1) Rx(x0), translation x3..5
            const double ct = cos(x[0]), st_ = sin(x[0]), cp = cos(x[1]), sp = sin(x[1]), cy = cos(x[2]), sy = sin(x[2]);
            double* X = J.X;
            X[0] = cy * cp; X[1] = cy * sp * st_ - sy * ct; X[2] = cy * sp * ct + sy * st_; X[3] = x[3];
            X[4] = sy * cp; X[5] = sy * sp * st_ + cy * ct; X[6] = sy * sp * ct - cy * st_; X[7] = x[4];
            X[8] = -sp;     X[9] = cp * st_;                X[10] = cp * ct;                X[11] = x[5];
            X[12] = 0.0; X[13] = 0.0; X[14] = 0.0; X[15] = 1.0;
            const double fval = sqrt(acc[27]) / (double)J.np;
            J.fval_perc = fval / J.fval_old;
            J.fval_old = fval;
            if (fval < J.fval_min) J.fval_min = fval;
            J.it += 1;
            const bool conv = J.fval_perc < 1.0 + J.tolp && J.fval_perc > 1.0 - J.tolp;
            go = !conv && J.it < J.max_it;
        }
    }
    J.active = go;
    if (go) atomicAdd(n_active, 1);
}

// M = transform(P, X) (xyz only: M's normals are never read).
__global__ void __launch_bounds__(PT_THREADS) icp_move_kernel(const IcpJob* __restrict__ jobs, const float* __restrict__ P,
                                                              float4* __restrict__ M)
{
    const IcpJob& J = jobs[blockIdx.y];
    const int i = blockIdx.x * PT_THREADS + threadIdx.x;
    if (!J.active || i >= J.np) return;
    float b[3];
    transform_pt(J.X, P + (J.soff + i) * 6, b, false);
    M[J.soff + i] = make_float4(b[0], b[1], b[2], 0.0f);
}

// cvRound: round half to even
inline int cv_round(double v) { return (int)std::nearbyint(v); }

}  // namespace

// Checks the parameters and the status-0 jobs (n_src, n_tgt); fills in the defaults.
int icp_check(const char* who, const p2p_icp_params* params, const p2p_icp_input* in, int n_jobs, p2p_icp_params& P)
{
    P = params ? *params : p2p_icp_params{100, 0.005f, 2.5f, 2};
    if (P.num_levels < 1 || P.num_levels > P2P_ICP_MAX_LEVELS || P.max_iterations < 1 || !std::isfinite(P.tolerance) ||
        !std::isfinite(P.rejection_scale)) {
        set_error("%s: ICP parameters max_iterations %d, tolerance %g, rejection_scale %g, num_levels %d (1..%d levels, >= 1 iteration, "
                  "finite tolerance and rejection scale)", who, P.max_iterations, (double)P.tolerance, (double)P.rejection_scale,
                  P.num_levels, P2P_ICP_MAX_LEVELS);
        return P2P_ERR_INVALID_ARG;
    }
    for (int j = 0; j < n_jobs; ++j) {
        const p2p_icp_input& R = in[j];
        if (R.status != 0) continue;
        if (R.n_src < 1 || R.n_tgt < 1 || R.n_src > 0x7fffffff || R.n_tgt > 0x7fffffff || R.src_offset < 0 || R.tgt_offset < 0 ||
            cv_round((double)R.n_src / (double)(1 << (P.num_levels - 1))) == 0) {
            set_error("%s: job %d: %lld source / %lld target points at offsets %lld / %lld (at least one target point, and enough source "
                      "points for %d pyramid levels)", who, j, (long long)R.n_src, (long long)R.n_tgt, (long long)R.src_offset,
                      (long long)R.tgt_offset, P.num_levels);
            return P2P_ERR_INVALID_ARG;
        }
    }
    return P2P_OK;
}

// The ICP of n_jobs records over device point arrays S (source) and T (target) with the offsets of the records; fills out.
int icp_run(Ctx& X, const p2p_icp_input* in, int n_jobs, const float* S, const float* T, const p2p_icp_params& P, p2p_icp_result* out)
{
    hipStream_t st = X.stream;
    const bool brute = dev_env("P2P_ICP_BRUTE") != nullptr;     // development twin: brute-force nearest neighbour
    const char* ce = dev_env("P2P_ICP_CHECK_EVERY");            // development twin: A/B of the stop-check interval
    const int check_every = ce ? std::max(1, atoi(ce)) : CHECK_EVERY;
    std::vector<IcpJob> hj(n_jobs);
    int64_t tot_n = 0, tot_m = 0;
    int max_n = 1, max_m = 1;
    for (int j = 0; j < n_jobs; ++j) {
        IcpJob& J = hj[j];
        std::memset(&J, 0, sizeof(J));
        J.status = in[j].status;
        J.keep_all = !(P.rejection_scale > 0.0f);
        if (J.status != 0) continue;
        J.n = (int)in[j].n_src; J.m = (int)in[j].n_tgt;
        J.soff = tot_n; J.toff = tot_m; J.coff = tot_m + 2 * j;
        J.in_s = in[j].src_offset; J.in_t = in[j].tgt_offset;
        tot_n += J.n; tot_m += J.m;
        max_n = std::max(max_n, J.n); max_m = std::max(max_m, J.m);
    }
    const int L = P.num_levels;
    // level constants, index [li][job], li = 0 for the coarsest level (l = L - 1)
    std::vector<IcpLevel> lv((size_t)L * n_jobs);
    std::vector<int> max_it(L, 0), max_np(L, 1), max_nq(L, 1);
    for (int li = 0; li < L; ++li) {
        const int l = L - 1 - li;
        for (int j = 0; j < n_jobs; ++j) {
            IcpLevel& V = lv[(size_t)li * n_jobs + j];
            std::memset(&V, 0, sizeof(V));
            if (hj[j].status != 0) continue;
            const int n = hj[j].n, m = hj[j].m;
            const int samples = cv_round((double)n / (double)(1 << l));
            V.step = cv_round((double)n / (double)samples);
            V.np = n / V.step;
            V.nq = m / V.step;
            V.tolp = (double)P.tolerance * (double)((l + 1) * (l + 1));
            V.max_it = cv_round((double)P.max_iterations / (double)(l + 1));
            max_it[li] = std::max(max_it[li], V.max_it);
            max_np[li] = std::max(max_np[li], V.np);
            max_nq[li] = std::max(max_nq[li], V.nq);
        }
    }
    DevBuf djobs, dlv, dS0, dT0, dP, dM, dQ, dqs, dqcell, dkeys, djidx, dd2, dcnt, dstart, dcur, dact;
    int rc;
    const int64_t nn = std::max<int64_t>(tot_n, 1), mm = std::max<int64_t>(tot_m, 1), cells = tot_m + 2 * (int64_t)n_jobs + 1;
    int max_iters = 1;
    for (int v : max_it) max_iters = std::max(max_iters, v);
    if ((rc = djobs.reserve(sizeof(IcpJob) * n_jobs)) || (rc = dlv.reserve(sizeof(IcpLevel) * lv.size())) ||
        (rc = dS0.reserve(nn * 24)) || (rc = dT0.reserve(mm * 24)) || (rc = dP.reserve(nn * 24)) || (rc = dM.reserve(nn * 16)) ||
        (rc = dQ.reserve(mm * 24)) || (rc = dqs.reserve(mm * 16)) || (rc = dqcell.reserve(mm * 4)) || (rc = dkeys.reserve(mm * 8)) ||
        (rc = djidx.reserve(nn * 4)) || (rc = dd2.reserve(nn * 4)) || (rc = dcnt.reserve(cells * 4)) || (rc = dstart.reserve(cells * 4)) ||
        (rc = dcur.reserve(cells * 4)) || (rc = dact.reserve(sizeof(int) * (L * (size_t)max_iters))))
        return rc;
    IcpJob* J = djobs.as<IcpJob>();
    HIP_TRY(hipMemcpyAsync(J, hj.data(), sizeof(IcpJob) * n_jobs, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dlv.p, lv.data(), sizeof(IcpLevel) * lv.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(dact.p, 0, sizeof(int) * (L * (size_t)max_iters), st));
    // (the caller's arrays are read in place through the input offsets; S0 / T0 are packed without the gaps of status != 0 records)
    icp_stats_kernel<<<n_jobs, 64, 0, st>>>(J, S, T);
    HIP_TRY(hipGetLastError());
    icp_normalise_kernel<<<dim3((std::max(max_n, max_m) + PT_THREADS - 1) / PT_THREADS, n_jobs, 2), PT_THREADS, 0, st>>>(
        J, S, T, dS0.as<float>(), dT0.as<float>());
    HIP_TRY(hipGetLastError());
    const unsigned jb = (unsigned)((n_jobs + 63) / 64);
    std::vector<int> act(1);
    for (int li = 0; li < L; ++li) {
        icp_level_kernel<<<jb, 64, 0, st>>>(J, n_jobs, dlv.as<IcpLevel>() + (size_t)li * n_jobs, L - 1 - li);
        HIP_TRY(hipGetLastError());
        const dim3 gp((max_np[li] + PT_THREADS - 1) / PT_THREADS, n_jobs), gq((max_nq[li] + PT_THREADS - 1) / PT_THREADS, n_jobs);
        const dim3 gs(std::max(gp.x, gq.x), n_jobs, 2);
        icp_sample_kernel<<<gs, PT_THREADS, 0, st>>>(J, dS0.as<float>(), dT0.as<float>(), dP.as<float>(), dM.as<float4>(), dQ.as<float>());
        HIP_TRY(hipGetLastError());
        if (!brute) {
            icp_grid_bbox_kernel<<<n_jobs, JOB_THREADS, 0, st>>>(J, dQ.as<float>(), dcnt.as<int>());
            HIP_TRY(hipGetLastError());
            icp_grid_count_kernel<<<gq, PT_THREADS, 0, st>>>(J, dQ.as<float>(), dqcell.as<int>(), dcnt.as<int>());
            HIP_TRY(hipGetLastError());
            icp_grid_scan_kernel<<<n_jobs, JOB_THREADS, 0, st>>>(J, dcnt.as<int>(), dstart.as<int>(), dcur.as<int>());
            HIP_TRY(hipGetLastError());
            icp_grid_scatter_kernel<<<gq, PT_THREADS, 0, st>>>(J, dQ.as<float>(), dqcell.as<int>(), dcur.as<int>(), dqs.as<float4>());
            HIP_TRY(hipGetLastError());
        }
        int* actv = dact.as<int>() + (size_t)li * max_iters;
        for (int it = 0; it < max_it[li]; ++it) {
            if (brute)
                icp_nn_brute_kernel<<<gp, PT_THREADS, 0, st>>>(J, dM.as<float4>(), dQ.as<float>(), djidx.as<int>(), dd2.as<float>());
            else
                icp_nn_grid_kernel<<<gp, PT_THREADS, 0, st>>>(J, dM.as<float4>(), dqs.as<float4>(), dstart.as<int>(), djidx.as<int>(),
                                                             dd2.as<float>());
            HIP_TRY(hipGetLastError());
            icp_select_kernel<<<n_jobs, JOB_THREADS, 0, st>>>(J, dd2.as<float>(), dkeys.as<unsigned long long>(), P.rejection_scale);
            HIP_TRY(hipGetLastError());
            icp_picky_kernel<<<gp, PT_THREADS, 0, st>>>(J, djidx.as<int>(), dd2.as<float>(), dkeys.as<unsigned long long>());
            HIP_TRY(hipGetLastError());
            icp_solve_kernel<<<n_jobs, JOB_THREADS, 0, st>>>(J, dP.as<float>(), dQ.as<float>(), dkeys.as<unsigned long long>(), actv + it);
            HIP_TRY(hipGetLastError());
            icp_move_kernel<<<gp, PT_THREADS, 0, st>>>(J, dP.as<float>(), dM.as<float4>());
            HIP_TRY(hipGetLastError());
            if ((it + 1) % check_every == 0 && it + 1 < max_it[li]) {       // every job done: stop queueing the level
                HIP_TRY(hipMemcpyAsync(act.data(), actv + it, sizeof(int), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                if (act[0] == 0) break;
            }
        }
        icp_level_end_kernel<<<jb, 64, 0, st>>>(J, n_jobs);
        HIP_TRY(hipGetLastError());
    }
    icp_finish_kernel<<<jb, 64, 0, st>>>(J, n_jobs);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hj.data(), J, sizeof(IcpJob) * n_jobs, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int j = 0; j < n_jobs; ++j) {
        const IcpJob& H = hj[j];
        p2p_icp_result& R = out[j];
        std::memset(&R, 0, sizeof(R));
        R.status = H.status;
        for (int k = 0; k < 16; ++k) R.pose[k] = (k % 5 == 0) ? 1.0 : 0.0;
        if (H.status != 0) continue;
        for (int l = 0; l < L; ++l) {
            R.iterations[l] = H.iterations[l];
            R.pairs[l] = H.pairs_lv[l];
            R.fval_min[l] = H.fval_min_lv[l];
        }
        R.scale = H.scale;
        for (int q = 0; q < 3; ++q) R.mean_avg[q] = H.mean_avg[q];
        for (int k = 0; k < 16; ++k) R.pose[k] = H.pose[k];
    }
    return P2P_OK;
}

int refine_chain(const char* who, p2p_ctx* ctx, const p2p_mesh* const* meshes, int n_meshes, const float* const* depth_images,
                 int n_images, const p2p_refine_job* jobs, int n_jobs, int height, int width, const p2p_icp_params* params,
                 p2p_refine_result* out, unsigned char* dinl, bool dev_inputs, DevBuf* dinl_alloc)
{
    if (!ctx || n_jobs < 0 || (n_jobs > 0 && !out)) {
        set_error("%s: bad arguments", who);
        return P2P_ERR_INVALID_ARG;
    }
    p2p_icp_params P;
    int rc;
    if ((rc = icp_check(who, params, nullptr, 0, P))) return rc;
    std::vector<p2p_icp_input> in(std::max(n_jobs, 1));
    IcpInputsStage S;
    if ((rc = icp_inputs_stage(who, ctx, meshes, n_meshes, depth_images, n_images, jobs, n_jobs, height, width, in.data(), S, dev_inputs)))
        return rc;
    if (n_jobs == 0) return P2P_OK;
    if ((rc = icp_check(who, params, in.data(), n_jobs, P))) return rc;
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    hipStream_t st = c->stream;
    std::vector<p2p_icp_result> icp(n_jobs);
    if ((rc = icp_run(*c, in.data(), n_jobs, S.dsrc.as<float>(), S.dtgt.as<float>(), P, icp.data()))) return rc;
    // tf = pose * [R | t_adjusted / 1000] (icp_refinement :91-93), R_ref = tf[:3,:3], t_ref = tf[:3,3] * 1000 (:466-467)
    std::vector<p2p_refine_job> rj(jobs, jobs + n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        p2p_refine_result& R = out[j];
        std::memset(&R, 0, sizeof(R));
        R.input = in[j];
        R.icp = icp[j];
        if (icp[j].status != 0) {
            for (int k = 0; k < 9; ++k) R.R[k] = jobs[j].R[k];
            for (int k = 0; k < 3; ++k) R.t[k] = jobs[j].t[k];
            continue;
        }
        double tf0[16] = {0}, tf[16];
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) tf0[4 * r + k] = jobs[j].R[3 * r + k];
            tf0[4 * r + 3] = in[j].t_adjusted[r] / 1000.0;
        }
        tf0[15] = 1.0;
        const double* A = icp[j].pose;
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) {
                double s = A[4 * a] * tf0[b];
                for (int k = 1; k < 4; ++k) s = s + A[4 * a + k] * tf0[4 * k + b];
                tf[4 * a + b] = s;
            }
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) R.R[3 * r + k] = rj[j].R[3 * r + k] = tf[4 * r + k];
            R.t[r] = rj[j].t[r] = tf[4 * r + 3] * 1000.0;
        }
    }
    // the score at the refined pose (the frames and union masks of the stage; every job is scored, the gated ones are zeroed below)
    const size_t HW = (size_t)height * width;
    DevBuf dof, dout, dz, dj;
    if ((rc = dof.reserve(sizeof(int) * n_jobs)) || (rc = dout.reserve(sizeof(p2p_depth_score) * n_jobs)) ||
        (dinl_alloc && (rc = dinl_alloc->reserve(n_jobs * HW))))
        return rc;
    if (dinl_alloc) dinl = dinl_alloc->as<unsigned char>();
    std::vector<p2p_depth_score> sc(n_jobs);
    HIP_TRY(hipMemcpyAsync(dof.p, S.slot_of.data(), sizeof(int) * n_jobs, hipMemcpyHostToDevice, st));
    if ((rc = score_into(*c, meshes, rj.data(), n_jobs, height, width, S.dimg.as<float>(), dof.as<int>(), S.dumask.as<unsigned char>(),
                         dinl, dout.as<p2p_depth_score>(), dz, dj)))
        return rc;
    HIP_TRY(hipMemcpyAsync(sc.data(), dout.p, sizeof(p2p_depth_score) * n_jobs, hipMemcpyDeviceToHost, st));
    for (int j = 0; j < n_jobs && dinl; ++j)
        if (icp[j].status != 0) HIP_TRY(hipMemsetAsync(dinl + j * HW, 0, HW, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int j = 0; j < n_jobs; ++j)
        if (icp[j].status == 0) out[j].score = sc[j];
    return P2P_OK;
}


}  // namespace p2p

using namespace p2p;

extern "C" {

int p2p_icp_batch(p2p_ctx* ctx, const p2p_icp_input* inputs, int n_jobs, const float* src_points, const float* tgt_points,
                  const p2p_icp_params* params, p2p_icp_result* out)
{
    const char* who = "p2p_icp_batch";
    if (!ctx || n_jobs < 0 || n_jobs > 65535 || (n_jobs > 0 && (!inputs || !out))) {
        set_error("%s: bad arguments", who);
        return P2P_ERR_INVALID_ARG;
    }
    p2p_icp_params P;
    int rc;
    if ((rc = icp_check(who, params, inputs, n_jobs, P))) return rc;
    int64_t ns = 0, nt = 0;     // extent of the caller's arrays that status-0 records name
    for (int j = 0; j < n_jobs; ++j)
        if (inputs[j].status == 0) {
            ns = std::max(ns, inputs[j].src_offset + inputs[j].n_src);
            nt = std::max(nt, inputs[j].tgt_offset + inputs[j].n_tgt);
        }
    if ((ns > 0 && !src_points) || (nt > 0 && !tgt_points)) {
        set_error("%s: null point buffer", who);
        return P2P_ERR_INVALID_ARG;
    }
    if (n_jobs == 0) return P2P_OK;
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    HIP_TRY(hipSetDevice(c->device));
    DevBuf ds, dt;
    if ((rc = ds.reserve(std::max<int64_t>(ns, 1) * 24)) || (rc = dt.reserve(std::max<int64_t>(nt, 1) * 24))) return rc;
    if (ns > 0) HIP_TRY(hipMemcpyAsync(ds.p, src_points, ns * 24, hipMemcpyHostToDevice, c->stream));
    if (nt > 0) HIP_TRY(hipMemcpyAsync(dt.p, tgt_points, nt * 24, hipMemcpyHostToDevice, c->stream));
    return icp_run(*c, inputs, n_jobs, ds.as<float>(), dt.as<float>(), P, out);
}

int p2p_refine_depth_batch(p2p_ctx* ctx, const p2p_mesh* const* meshes, int n_meshes, const float* const* depth_images, int n_images,
                           const p2p_refine_job* jobs, int n_jobs, int height, int width, const p2p_icp_params* params,
                           p2p_refine_result* out, unsigned char* inlier_masks)
{
    const char* who = "p2p_refine_depth_batch";
    DevBuf dinl;       // the inlier masks on the device, allocated by the chain once its checks have passed
    int rc = refine_chain(who, ctx, meshes, n_meshes, depth_images, n_images, jobs, n_jobs, height, width, params, out, nullptr, false,
                          inlier_masks ? &dinl : nullptr);
    if (rc || !inlier_masks || n_jobs == 0) return rc;
    hipStream_t st = reinterpret_cast<Ctx*>(ctx)->stream;
    HIP_TRY(hipMemcpyAsync(inlier_masks, dinl.p, (size_t)n_jobs * height * width, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return P2P_OK;
}

}  // extern "C"
