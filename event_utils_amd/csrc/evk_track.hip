// Camera tracking (include/evk.h, "Camera tracking"): 6-DoF registration of the 3-D points of a reference view to a time surface, the
// tracking step of ESVO (Zhou et al., T-RO 2021, section V).
//
//   k_track_terms       a lane per point, four points a lane, B poses on blockIdx.y (the poses are kernel arguments: nothing is
//                       copied to the device per evaluation).  The 29 sums stay in registers; the 64 lanes of a wave are added by a
//                       scan on DPP (no LDS instruction), the four waves through 928 bytes of LDS, and the workgroup writes one row.
//   k_track_rows        adds the rows of a pose: eight chains of every eighth row, each in index order, then the eight in order
//   k_track_residuals   the per-point r, J and valid flag of one pose, and no sums
//   evk_track_register  the Levenberg-Marquardt loop on the host: two launches and one read-back of 29 doubles per evaluation
//
// All arithmetic is double with one rounding per operation (-ffp-contract=off), so a per-point value is the bits of the numpy
// restatement; the sums follow one fixed tree that depends on m only, so a result repeats bit for bit.  No atomics.
#include <math.h>

#include "evk_common.h"

namespace evk {

constexpr int kTrackThreads = 256;
constexpr int kTrackPer = 4;                                            // points per lane
constexpr int kTrackSpan = kTrackThreads * kTrackPer;                   // points per workgroup row
constexpr int kTrackSums = EVK_TRACK_SUMS;                              // 21 of A, 6 of g, c, n
constexpr int kTrackWaves = kTrackThreads / EVK_WAVE;
constexpr int kTrackFan = kTrackThreads / 32;                           // chains of rows in k_track_rows

struct TrackArgs {
    const double *points;
    const float *surface;
    int64_t m;
    int h, w, huber;
    double fx, fy, cx, cy, delta;
    double *rows, *r, *jac;
    uint8_t *valid;
    double pose[EVK_TRACK_MAX_POSES][12];
};

struct TrackPoint {
    double r, j[6];
    bool ok;
};

__device__ __forceinline__ bool track_finite(double v) { return v - v == 0.0; }

// the definition, in its order of operations; the values of a point that is not valid are not used
__device__ __forceinline__ TrackPoint track_point(const TrackArgs &p, const double (&T)[12], int64_t i) {
    TrackPoint o;
    bool ok = i < p.m;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (ok) px = p.points[3 * i], py = p.points[3 * i + 1], pz = p.points[3 * i + 2];
    const double X = ((T[0] * px + T[1] * py) + T[2] * pz) + T[9];
    const double Y = ((T[3] * px + T[4] * py) + T[5] * pz) + T[10];
    const double Z = ((T[6] * px + T[7] * py) + T[8] * pz) + T[11];
    ok = ok && track_finite(X) && track_finite(Y) && track_finite(Z) && Z > 0.0;
    const double u = p.fx * (X / Z) + p.cx, v = p.fy * (Y / Z) + p.cy;
    ok = ok && u >= 0.0 && u < (double)(p.w - 1) && v >= 0.0 && v < (double)(p.h - 1);          // (a NaN fails)
    const double fu = floor(u), fv = floor(v);
    float s00 = 0.f, s01 = 0.f, s10 = 0.f, s11 = 0.f;
    if (ok) {                                                           // 0 <= x0 <= w - 2, 0 <= y0 <= h - 2
        const float *s = p.surface + (int64_t)(int)fv * p.w + (int)fu;
        s00 = s[0], s01 = s[1], s10 = s[p.w], s11 = s[p.w + 1];
    }
    const double S00 = (double)s00, S01 = (double)s01, S10 = (double)s10, S11 = (double)s11;
    ok = ok && track_finite(S00) && track_finite(S01) && track_finite(S10) && track_finite(S11);
    const double a = u - fu, b = v - fv, a1 = 1.0 - a, b1 = 1.0 - b;
    o.r = b1 * (a1 * S00 + a * S01) + b * (a1 * S10 + a * S11);
    const double gx = b1 * (S01 - S00) + b * (S11 - S10), gy = a1 * (S10 - S00) + a * (S11 - S01);
    const double qx = gx * p.fx, qy = gy * p.fy;
    o.j[0] = qx / Z, o.j[1] = qy / Z, o.j[2] = -((qx * X + qy * Y) / (Z * Z));
    o.j[3] = Y * o.j[2] - Z * o.j[1], o.j[4] = Z * o.j[0] - X * o.j[2], o.j[5] = X * o.j[1] - Y * o.j[0];
    o.ok = ok;
    return o;
}

// v + the value of the lane that CTRL names, 0.0 where there is none or the row is masked out.  All 64 lanes must be active.
template <int CTRL, int ROWS>
__device__ __forceinline__ double track_dpp_add(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWS, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWS, 0xf, false);
    return v + __hiloint2double(hi, lo);
}
// the inclusive scan of evk_common.h on doubles: lane 63 ends with the sum of the wave, by one fixed tree
__device__ __forceinline__ double track_wave_sum(double v) {
    v = track_dpp_add<0x111, 0xf>(v);                                   // row_shr:1
    v = track_dpp_add<0x112, 0xf>(v);                                   // row_shr:2
    v = track_dpp_add<0x114, 0xf>(v);                                   // row_shr:4
    v = track_dpp_add<0x118, 0xf>(v);                                   // row_shr:8
    v = track_dpp_add<0x142, 0xa>(v);                                   // row_bcast:15 into rows 1 and 3
    v = track_dpp_add<0x143, 0xc>(v);                                   // row_bcast:31 into rows 2 and 3
    return v;
}

__global__ void __launch_bounds__(kTrackThreads) k_track_terms(TrackArgs p, int groups) {
    __shared__ double part[kTrackWaves][kTrackSums];
    const int pose = blockIdx.y;
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = p.pose[pose][k];
    double acc[kTrackSums];
#pragma unroll
    for (int k = 0; k < kTrackSums; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int q = 0; q < kTrackPer; ++q) {
        const TrackPoint o = track_point(p, T, (int64_t)blockIdx.x * kTrackSpan + q * kTrackThreads + threadIdx.x);
        const double ar = fabs(o.r);
        const bool tail = p.huber && ar > p.delta;
        const double w = tail ? p.delta / ar : 1.0;
        const double rho = tail ? p.delta * (2.0 * ar - p.delta) : o.r * o.r;
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const double wj = w * o.j[i];
#pragma unroll
            for (int j = i; j < 6; ++j, ++k) acc[k] += o.ok ? wj * o.j[j] : 0.0;
            acc[21 + i] += o.ok ? wj * o.r : 0.0;
        }
        acc[27] += o.ok ? rho : 0.0;
        acc[28] += o.ok ? 1.0 : 0.0;
    }
    // (no lane has left: the scans need all 64)
    const int lane = threadIdx.x & (EVK_WAVE - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kTrackSums; ++k) {
        const double s = track_wave_sum(acc[k]);
        if (lane == EVK_WAVE - 1) part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < kTrackSums) {
        const int k = threadIdx.x;
        p.rows[((int64_t)pose * groups + blockIdx.x) * kTrackSums + k] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
    }
}

// the rows of a pose: lane (j, k) adds sum k of the rows g = j, j + 8, j + 16, ... in order (eight chains of loads in flight, not
// one), then the eight are added in order
__global__ void __launch_bounds__(kTrackThreads) k_track_rows(const double *__restrict__ rows, int groups, double *__restrict__ sums) {
    __shared__ double part[kTrackFan][kTrackSums];
    const int k = threadIdx.x & 31, j = threadIdx.x >> 5;
    if (k < kTrackSums) {
        const double *row = rows + (int64_t)blockIdx.x * groups * kTrackSums + k;
        double s = 0.0;
#pragma unroll 4
        for (int g = j; g < groups; g += kTrackFan) s += row[(int64_t)g * kTrackSums];
        part[j][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < kTrackSums) {
        double s = part[0][threadIdx.x];
#pragma unroll
        for (int q = 1; q < kTrackFan; ++q) s += part[q][threadIdx.x];
        sums[(int64_t)blockIdx.x * kTrackSums + threadIdx.x] = s;
    }
}

__global__ void __launch_bounds__(kTrackThreads) k_track_residuals(TrackArgs p) {
    const int64_t i = (int64_t)blockIdx.x * kTrackThreads + threadIdx.x;
    if (i >= p.m) return;
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = p.pose[0][k];
    const TrackPoint o = track_point(p, T, i);
    const double nan = __builtin_nan("");
    p.r[i] = o.ok ? o.r : nan;
#pragma unroll
    for (int k = 0; k < 6; ++k) p.jac[6 * i + k] = o.ok ? o.j[k] : nan;
    p.valid[i] = o.ok ? 1 : 0;
}

static inline bool track_finite_host(double v) { return v - v == 0.0; }
static inline int track_groups(int64_t m) { return (int)((m + kTrackSpan - 1) / kTrackSpan); }

// the checks every entry shares; fills `p` (all but the outputs)
static bool track_args(TrackArgs &p, const double *points, int64_t m, const float *surface, int h, int w, double fx, double fy, double cx,
                       double cy, const double *poses, int nb, int loss, double delta) {
    if (!points || !surface || !poses || m < 1 || m > 0x7FFFFFFFll || h < 2 || w < 2 || (int64_t)h * w > 0x7FFFFFFFll) return false;
    if (nb < 1 || nb > EVK_TRACK_MAX_POSES || (loss != EVK_TRACK_L2 && loss != EVK_TRACK_HUBER)) return false;
    if (!track_finite_host(fx) || !track_finite_host(fy) || !track_finite_host(cx) || !track_finite_host(cy) || !(fx > 0.0) || !(fy > 0.0))
        return false;
    if (loss == EVK_TRACK_HUBER && !(delta > 0.0 && track_finite_host(delta))) return false;
    for (int k = 0; k < 12 * nb; ++k)
        if (!track_finite_host(poses[k])) return false;
    p = TrackArgs{};
    p.points = points, p.surface = surface, p.m = m, p.h = h, p.w = w, p.huber = loss == EVK_TRACK_HUBER;
    p.fx = fx, p.fy = fy, p.cx = cx, p.cy = cy, p.delta = p.huber ? delta : 0.0;
    for (int b = 0; b < nb; ++b)
        for (int k = 0; k < 12; ++k) p.pose[b][k] = poses[12 * b + k];
    return true;
}

// the rows of every pose of `p` into scratch, their sums into `sums` (device)
static int track_launch(TrackArgs &p, int nb, void *scratch, double *sums, hipStream_t s) {
    const int groups = track_groups(p.m);
    p.rows = static_cast<double *>(scratch);
    k_track_terms<<<dim3((unsigned)groups, (unsigned)nb), kTrackThreads, 0, s>>>(p, groups);
    k_track_rows<<<nb, kTrackThreads, 0, s>>>(p.rows, groups, sums);
    return launch_status();
}

// ---- the host side of the loop: a 6 x 6 Cholesky solve and the exponential of se(3) ------------------------------------------------

// (A + lambda diag A) d = -g with A's upper triangle row-major in `a`; false when the matrix is not positive definite
static bool track_solve(const double *a, const double *g, double lambda, double *d) {
    double M[6][6], L[6][6] = {};
    int k = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j, ++k) M[i][j] = M[j][i] = a[k];
    for (int i = 0; i < 6; ++i) M[i][i] = M[i][i] + lambda * M[i][i];
    for (int j = 0; j < 6; ++j) {
        double s = M[j][j];
        for (int q = 0; q < j; ++q) s -= L[j][q] * L[j][q];
        if (!(s > 0.0) || !track_finite_host(s)) return false;
        L[j][j] = sqrt(s);
        for (int i = j + 1; i < 6; ++i) {
            double t = M[i][j];
            for (int q = 0; q < j; ++q) t -= L[i][q] * L[j][q];
            L[i][j] = t / L[j][j];
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double t = -g[i];
        for (int q = 0; q < i; ++q) t -= L[i][q] * y[q];
        y[i] = t / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double t = y[i];
        for (int q = i + 1; q < 6; ++q) t -= L[q][i] * d[q];
        d[i] = t / L[i][i];
        if (!track_finite_host(d[i])) return false;
    }
    return true;
}

// out = exp(xi^) T, xi = (upsilon, omega), T = (R row-major, t)
static void track_exp_left(const double *xi, const double *T, double *out) {
    const double wx = xi[3], wy = xi[4], wz = xi[5];
    const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
    double A, B, C;
    if (th2 < 1e-8) {                                                   // (the closed forms cancel: 1 - cos th is 0 below 1e-8)
        A = 1.0 - th2 / 6.0, B = 0.5 - th2 / 24.0, C = 1.0 / 6.0 - th2 / 120.0;
    } else {
        const double sh = sin(0.5 * th);
        A = sin(th) / th, B = (2.0 * sh * sh) / th2, C = (th - sin(th)) / (th2 * th);
    }
    const double W[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
    double W2[3][3], R[3][3], V[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W2[i][j] = (W[i][0] * W[0][j] + W[i][1] * W[1][j]) + W[i][2] * W[2][j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double e = i == j ? 1.0 : 0.0;
            R[i][j] = (e + A * W[i][j]) + B * W2[i][j];
            V[i][j] = (e + B * W[i][j]) + C * W2[i][j];
        }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) out[3 * i + j] = (R[i][0] * T[j] + R[i][1] * T[3 + j]) + R[i][2] * T[6 + j];
        out[9 + i] = ((R[i][0] * T[9] + R[i][1] * T[10]) + R[i][2] * T[11]) + ((V[i][0] * xi[0] + V[i][1] * xi[1]) + V[i][2] * xi[2]);
    }
}

}  // namespace evk

using namespace evk;

extern "C" int64_t evk_track_scratch_bytes(int64_t m, int nb) {
    if (m < 1 || m > 0x7FFFFFFFll || nb < 1 || nb > EVK_TRACK_MAX_POSES) return EVK_EINVAL;
    return ((int64_t)track_groups(m) + 1) * nb * kTrackSums * (int64_t)sizeof(double);
}

extern "C" int evk_track_terms(const double *points, int64_t m, const float *surface, int h, int w, double fx, double fy, double cx,
                               double cy, const double *poses, int nb, int loss, double delta, void *scratch, double *sums, void *stream) {
    TrackArgs p;
    if (!scratch || !sums || !track_args(p, points, m, surface, h, w, fx, fy, cx, cy, poses, nb, loss, delta)) return EVK_EINVAL;
    return track_launch(p, nb, scratch, sums, (hipStream_t)stream);
}

extern "C" int evk_track_residuals(const double *points, int64_t m, const float *surface, int h, int w, double fx, double fy, double cx,
                                   double cy, const double *pose, double *r, double *jac, void *valid, void *stream) {
    TrackArgs p;
    if (!r || !jac || !valid || !track_args(p, points, m, surface, h, w, fx, fy, cx, cy, pose, 1, EVK_TRACK_L2, 0.0)) return EVK_EINVAL;
    p.r = r, p.jac = jac, p.valid = static_cast<uint8_t *>(valid);
    k_track_residuals<<<(unsigned)((m + kTrackThreads - 1) / kTrackThreads), kTrackThreads, 0, (hipStream_t)stream>>>(p);
    return launch_status();
}

extern "C" int evk_track_register(const double *points, int64_t m, const float *surface, int h, int w, double fx, double fy, double cx,
                                  double cy, double *pose, int loss, double delta, int max_evals, int64_t min_points, double step_tol,
                                  void *scratch, double *cost, int64_t *n_valid, int *evaluations, int *status, void *stream) {
    TrackArgs p;
    if (!scratch || !cost || !n_valid || !evaluations || !status || max_evals < 1 || min_points < 1 || !(step_tol >= 0.0) ||
        !track_args(p, points, m, surface, h, w, fx, fy, cx, cy, pose, 1, loss, delta))
        return EVK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    double *sums = static_cast<double *>(scratch) + (int64_t)track_groups(m) * kTrackSums;        // behind the rows
    double T[12], cur[kTrackSums], cand[kTrackSums], Tc[12], d[6];
    const auto evaluate = [&](const double *at, double *out) -> int {
        for (int k = 0; k < 12; ++k) p.pose[0][k] = at[k];
        if (int rc = track_launch(p, 1, scratch, sums, s)) return rc;
        hipError_t e = hipMemcpyAsync(out, sums, sizeof(double) * kTrackSums, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        return e == hipSuccess ? EVK_OK : (int)e;
    };
    for (int k = 0; k < 12; ++k) T[k] = pose[k];
    if (int rc = evaluate(T, cur)) return rc;
    int evals = 1, st = EVK_TRACK_MAX_EVALS;
    if (cur[28] < (double)min_points) {
        st = EVK_TRACK_LOST;
    } else {
        double lambda = 1e-3;
        while (evals < max_evals) {
            if (lambda > 1e6) {
                st = EVK_TRACK_STALLED;
                break;
            }
            if (!track_solve(cur, cur + 21, lambda, d)) {
                lambda = 10.0 * lambda;
                continue;
            }
            track_exp_left(d, T, Tc);
            bool finite = true;
            for (int k = 0; k < 12; ++k) finite = finite && track_finite_host(Tc[k]);
            if (!finite) {
                lambda = 10.0 * lambda;
                continue;
            }
            if (int rc = evaluate(Tc, cand)) return rc;
            ++evals;
            if (cand[28] >= (double)min_points && cand[27] / cand[28] < cur[27] / cur[28]) {
                for (int k = 0; k < 12; ++k) T[k] = Tc[k];
                for (int k = 0; k < kTrackSums; ++k) cur[k] = cand[k];
                lambda = fmax(lambda / 10.0, 1e-9);
                double n2 = 0.0;
                for (int k = 0; k < 6; ++k) n2 += d[k] * d[k];
                if (sqrt(n2) < step_tol) {
                    st = EVK_TRACK_CONVERGED;
                    break;
                }
            } else {
                lambda = 10.0 * lambda;
            }
        }
    }
    for (int k = 0; k < 12; ++k) pose[k] = T[k];
    *cost = cur[27], *n_valid = (int64_t)cur[28], *evaluations = evals, *status = st;
    return EVK_OK;
}
