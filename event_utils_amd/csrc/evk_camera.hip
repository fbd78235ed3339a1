// Camera calibration (include/evk.h, "Camera calibration"): lens distortion and its inverse, the forward
// (event) and inverse (image) rectification maps, the per-event look-up in the forward map and the remap of image planes through
// the inverse map.  Three kernels, one lane per point / event / output pixel, no LDS, no atomics but the rare OR into *bad, no
// scratch memory.  Every value is an IEEE double with one rounding per operation in the order evk.h states (-ffp-contract=off):
// `none` and `radtan` are the same bits as the numpy restatement (tests/_camera_np.py); `equidistant` calls atan and tan, which
// are the device library's.  The calibration travels as a kernel argument (CamParams, 200 bytes): no table, no upload.
#include <type_traits>

#include "evk_common.h"

namespace evk {

struct CamParams {
    double fx, fy, cx, cy;       // K
    double d[5];                 // radtan k1 k2 p1 p2 k3; equidistant k1 k2 k3 k4
    double m[9];                 // EVK_CAMERA_FORWARD: R; EVK_CAMERA_INVERSE: R^T (row-major)
    double gx, gy, ox, oy;       // new_K
    double tol;                  // pixels
    int iterations;
};

constexpr double CAM_SMALL_R = 1e-8;
constexpr double CAM_HALF_PI = 1.5707963267948966;          // the double nearest pi / 2

__device__ __forceinline__ void radtan_terms(const CamParams &c, double a, double b, double &rad, double &dx, double &dy) {
    const double aa = a * a, bb = b * b, ab = a * b;
    const double r2 = aa + bb;
    rad = 1.0 + r2 * (c.d[0] + r2 * (c.d[1] + r2 * c.d[4]));
    dx = (2.0 * c.d[2]) * ab + c.d[3] * (r2 + 2.0 * aa);
    dy = c.d[2] * (r2 + 2.0 * bb) + (2.0 * c.d[3]) * ab;
}

__device__ __forceinline__ double theta_d(const CamParams &c, double th) {
    const double th2 = th * th;
    return th * (1.0 + th2 * (c.d[0] + th2 * (c.d[1] + th2 * (c.d[2] + th2 * c.d[3]))));
}

template <int MODEL>
__device__ __forceinline__ void cam_distort(const CamParams &c, double a, double b, double &ad, double &bd) {
    if constexpr (MODEL == EVK_CAMERA_RADTAN) {
        double rad, dx, dy;
        radtan_terms(c, a, b, rad, dx, dy);
        ad = a * rad + dx, bd = b * rad + dy;
    } else if constexpr (MODEL == EVK_CAMERA_EQUIDISTANT) {
        const double r = sqrt(a * a + b * b);
        const double thd = theta_d(c, atan(r));
        const double s = r < CAM_SMALL_R ? 1.0 : thd / r;
        ad = a * s, bd = b * s;
    } else {
        ad = a, bd = b;
    }
}

// -> valid.  The iteration count is wave-uniform (a kernel argument): no lane leaves a loop early
template <int MODEL>
__device__ __forceinline__ bool cam_undistort(const CamParams &c, double ad, double bd, double &a, double &b) {
    bool ok = true;
    a = ad, b = bd;
    if constexpr (MODEL == EVK_CAMERA_RADTAN) {
        for (int it = 0; it < c.iterations; ++it) {
            double rad, dx, dy;
            radtan_terms(c, a, b, rad, dx, dy);
            const double icd = 1.0 / rad;
            a = (ad - dx) * icd, b = (bd - dy) * icd;
        }
    } else if constexpr (MODEL == EVK_CAMERA_EQUIDISTANT) {
        const double rd = sqrt(ad * ad + bd * bd);
        const double c3 = 3.0 * c.d[0], c5 = 5.0 * c.d[1], c7 = 7.0 * c.d[2], c9 = 9.0 * c.d[3];
        double th = rd;
        for (int it = 0; it < c.iterations; ++it) {
            const double th2 = th * th;
            const double f = theta_d(c, th) - rd;
            const double fp = 1.0 + th2 * (c3 + th2 * (c5 + th2 * (c7 + th2 * c9)));
            th = th - f / fp;
        }
        ok = th >= 0.0 && th < CAM_HALF_PI;
        // (tan of a lane that already failed is not used: its argument is kept inside the quadrant)
        const double s = rd < CAM_SMALL_R ? 1.0 : tan(ok ? th : 0.0) / rd;
        a = ad * s, b = bd * s;
    }
    ok = ok && __builtin_isfinite(a) && __builtin_isfinite(b);
    double ar, br;
    cam_distort<MODEL>(c, a, b, ar, br);
    return ok && fabs(c.fx * (ar - ad)) <= c.tol && fabs(c.fy * (br - bd)) <= c.tol;
}

__device__ __forceinline__ void cam_rotate(const CamParams &c, double a, double b, double &X, double &Y, double &Z) {
    X = (c.m[0] * a + c.m[1] * b) + c.m[2];
    Y = (c.m[3] * a + c.m[4] * b) + c.m[5];
    Z = (c.m[6] * a + c.m[7] * b) + c.m[8];
}

// pts: n interleaved (x, y) pairs, or NULL: point i is pixel (i % w, i / w) of the grid.  out: (2, n); valid: n bytes
template <int MODEL, int DIR>
__global__ void __launch_bounds__(EVK_BLOCK) k_camera_points(const double *__restrict__ pts, int64_t n, int w, CamParams c,
                                                           double *__restrict__ out, uint8_t *__restrict__ valid) {
    const int64_t i = (int64_t)blockIdx.x * EVK_BLOCK + threadIdx.x;
    if (i >= n) return;
    double x, y;
    if (pts) {
        x = pts[2 * i], y = pts[2 * i + 1];
    } else {
        const uint32_t row = (uint32_t)i / (uint32_t)w;
        x = (double)((uint32_t)i - row * (uint32_t)w), y = (double)row;
    }
    double u, v, X, Y, Z;
    bool ok;
    if constexpr (DIR == EVK_CAMERA_FORWARD) {
        double a, b;
        ok = cam_undistort<MODEL>(c, (x - c.cx) / c.fx, (y - c.cy) / c.fy, a, b);
        cam_rotate(c, a, b, X, Y, Z);
        ok = ok && Z > 0.0;
        u = c.gx * (X / Z) + c.ox, v = c.gy * (Y / Z) + c.oy;
    } else {
        cam_rotate(c, (x - c.ox) / c.gx, (y - c.oy) / c.gy, X, Y, Z);
        double ad, bd;
        cam_distort<MODEL>(c, X / Z, Y / Z, ad, bd);
        u = c.fx * ad + c.cx, v = c.fy * bd + c.cy;
        ok = Z > 0.0 && __builtin_isfinite(u) && __builtin_isfinite(v);
    }
    const double nan = __builtin_nan("");
    out[i] = ok ? u : nan;
    out[n + i] = ok ? v : nan;
    valid[i] = ok ? 1 : 0;
}

__device__ __forceinline__ void store_kind(void *dst, int kind, int64_t i, double v) {
    switch (kind) {
        case EVK_SELECT_I16: static_cast<int16_t *>(dst)[i] = (int16_t)v; break;
        case EVK_SELECT_I32: static_cast<int32_t *>(dst)[i] = (int32_t)v; break;
        case EVK_SELECT_I64: static_cast<int64_t *>(dst)[i] = (int64_t)v; break;
        case EVK_SELECT_F32: static_cast<float *>(dst)[i] = (float)v; break;
        default: static_cast<double *>(dst)[i] = v; break;
    }
}

// a raw coordinate as a pixel index below `size`: false for a value that is no integer, NaN, negative or >= size
template <typename T>
__device__ __forceinline__ bool pixel_index(T v, int size, int &out) {
    if constexpr (std::is_integral<T>::value) {
        if ((int64_t)v < 0 || (int64_t)v >= (int64_t)size) return false;
        out = (int)v;
    } else {
        const double d = (double)v;
        if (!(d >= 0.0 && d < (double)size) || d != trunc(d)) return false;
        out = (int)d;
    }
    return true;
}

// one lane per event: the entry (map[0, y, x], map[1, y, x]) of its pixel -> new coordinates (of kind out_kind) and a keep flag.
// A dropped event gets the coordinates 0.  The index y w + x is below h w <= 2^31 - 1 by pixel_index
template <typename T>
__global__ void __launch_bounds__(EVK_BLOCK) k_rectify_lookup(const T *__restrict__ xs, const T *__restrict__ ys, int64_t n,
                                                            const double *__restrict__ map, const uint8_t *__restrict__ mvalid, int h,
                                                            int w, int oh, int ow, int mode, int out_kind, void *__restrict__ ox,
                                                            void *__restrict__ oy, uint8_t *__restrict__ keep, uint32_t *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * EVK_BLOCK + threadIdx.x;
    if (i >= n) return;
    int xi = 0, yi = 0;
    const bool on = pixel_index(xs[i], w, xi) && pixel_index(ys[i], h, yi);
    double u = 0.0, v = 0.0;
    bool k = false;
    if (on) {
        const int64_t at = (int64_t)yi * w + xi;
        u = map[at], v = map[(int64_t)h * w + at];
        const bool ok = mvalid[at] != 0;
        if (mode == EVK_CAMERA_NEAREST) {
            u = rint(u) + 0.0, v = rint(v) + 0.0;          // (+ 0.0: a rounded -0.3 is the pixel 0, not -0)
            k = ok && u >= 0.0 && u < (double)ow && v >= 0.0 && v < (double)oh;
        } else {
            k = ok && u >= 0.0 && u <= (double)(ow - 1) && v >= 0.0 && v <= (double)(oh - 1);
        }
    } else if (bad) {
        atomicOr(bad, 1u);
    }
    store_kind(ox, out_kind, i, k ? u : 0.0);
    store_kind(oy, out_kind, i, k ? v : 0.0);
    keep[i] = k ? 1 : 0;
}

// one rounding of a double to the plane's dtype; uint8: half to even, then clamped to 0 .. 255 (NaN gives 0)
template <typename T>
__device__ __forceinline__ T to_plane(double v) {
    if constexpr (std::is_same<T, uint8_t>::value) {
        const double r = rint(v);
        return r > 0.0 ? (uint8_t)(r < 255.0 ? r : 255.0) : (uint8_t)0;
    } else {
        return (T)v;
    }
}

// one lane per output pixel; the map entry is read once and serves every plane
template <typename T>
__global__ void __launch_bounds__(EVK_BLOCK) k_remap_planes(const T *__restrict__ src, int64_t planes, int h, int w,
                                                          const double *__restrict__ map, const uint8_t *__restrict__ mvalid, int oh, int ow,
                                                          int interpolation, double fill, T *__restrict__ dst) {
    const int64_t ohw = (int64_t)oh * ow, hw = (int64_t)h * w;
    const int64_t i = (int64_t)blockIdx.x * EVK_BLOCK + threadIdx.x;
    if (i >= ohw) return;
    const double mx = map[i], my = map[ohw + i];
    const double sx = rint(mx), sy = rint(my);
    const bool ok = mvalid[i] != 0 && sx >= 0.0 && sx < (double)w && sy >= 0.0 && sy < (double)h;
    const T fill_t = to_plane<T>(fill);
    if (!ok) {
        for (int64_t p = 0; p < planes; ++p) dst[p * ohw + i] = fill_t;
        return;
    }
    if (interpolation == EVK_CAMERA_NEAREST) {
        const int64_t at = (int64_t)(int)sy * w + (int)sx;
        for (int64_t p = 0; p < planes; ++p) dst[p * ohw + i] = src[p * hw + at];
        return;
    }
    // the nearest pixel is on the sensor, so x0 is -1 .. w - 1 and y0 is -1 .. h - 1: a tap off the sensor takes the fill value
    const double x0 = floor(mx), y0 = floor(my);
    const double a = mx - x0, b = my - y0;
    const double a1 = 1.0 - a, b1 = 1.0 - b;
    const int xi = (int)x0, yi = (int)y0;
    const bool l = xi >= 0, r = xi + 1 < w, t = yi >= 0, u = yi + 1 < h;
    const int64_t at = (int64_t)yi * w + xi;
    const double f = (double)fill_t;
    for (int64_t p = 0; p < planes; ++p) {
        const T *s = src + p * hw;
        const double v00 = t && l ? (double)s[at] : f, v01 = t && r ? (double)s[at + 1] : f;
        const double v10 = u && l ? (double)s[at + w] : f, v11 = u && r ? (double)s[at + w + 1] : f;
        dst[p * ohw + i] = to_plane<T>(b1 * (a1 * v00 + a * v01) + b * (a1 * v10 + a * v11));
    }
}

static bool positive(double v) { return v > 0.0 && v < 1.0 / 0.0; }
static bool is_finite(double v) { return v - v == 0.0; }

template <int MODEL>
static void launch_points(int direction, const double *pts, int64_t n, int w, const CamParams &c, double *out, uint8_t *valid,
                          hipStream_t s) {
    const unsigned grid = (unsigned)((n + EVK_BLOCK - 1) / EVK_BLOCK);
    if (direction == EVK_CAMERA_FORWARD) k_camera_points<MODEL, EVK_CAMERA_FORWARD><<<grid, EVK_BLOCK, 0, s>>>(pts, n, w, c, out, valid);
    else k_camera_points<MODEL, EVK_CAMERA_INVERSE><<<grid, EVK_BLOCK, 0, s>>>(pts, n, w, c, out, valid);
}

}  // namespace evk

using namespace evk;

extern "C" int evk_camera_points(int model, int direction, const double *points, int64_t n, int h, int w, const double *host_params,
                                 int iterations, double tolerance, double *out, void *valid, void *stream) {
    if (model < EVK_CAMERA_NONE || model > EVK_CAMERA_EQUIDISTANT || (direction != EVK_CAMERA_FORWARD && direction != EVK_CAMERA_INVERSE) ||
        n < 0 || n >= ((int64_t)1 << 31) * EVK_BLOCK || h < 0 || w < 0 || (int64_t)h * w > INT32_MAX || !host_params || iterations < 1 ||
        !(tolerance >= 0.0) || !out || !valid || (!points && n != (int64_t)h * w))
        return EVK_EINVAL;
    CamParams c;
    const double *q = host_params;
    c.fx = q[0], c.fy = q[1], c.cx = q[2], c.cy = q[3];
    for (int k = 0; k < 5; ++k) c.d[k] = q[4 + k];
    for (int k = 0; k < 9; ++k) c.m[k] = q[9 + k];
    c.gx = q[18], c.gy = q[19], c.ox = q[20], c.oy = q[21];
    c.tol = tolerance, c.iterations = iterations;
    if (!positive(c.fx) || !positive(c.fy) || !positive(c.gx) || !positive(c.gy)) return EVK_EINVAL;
    for (int k = 2; k < 22; ++k)
        if (k != 18 && k != 19 && !is_finite(q[k])) return EVK_EINVAL;
    if (n == 0) return EVK_OK;
    hipStream_t s = (hipStream_t)stream;
    uint8_t *vb = static_cast<uint8_t *>(valid);
    if (model == EVK_CAMERA_RADTAN) launch_points<EVK_CAMERA_RADTAN>(direction, points, n, w, c, out, vb, s);
    else if (model == EVK_CAMERA_EQUIDISTANT) launch_points<EVK_CAMERA_EQUIDISTANT>(direction, points, n, w, c, out, vb, s);
    else launch_points<EVK_CAMERA_NONE>(direction, points, n, w, c, out, vb, s);
    return launch_status();
}

extern "C" int evk_camera_rectify_lookup(int coord_kind, const void *x, const void *y, int64_t n, const double *map, const void *map_valid,
                                         int h, int w, int out_h, int out_w, int mode, int out_kind, void *out_x, void *out_y, void *keep,
                                         void *bad, void *stream) {
    if (coord_kind < EVK_SELECT_I16 || coord_kind > EVK_SELECT_F64 || out_kind < EVK_SELECT_I16 || out_kind > EVK_SELECT_F64 || n < 0 ||
        n >= ((int64_t)1 << 31) * EVK_BLOCK || h < 0 || w < 0 || out_h < 0 || out_w < 0 || (int64_t)h * w > INT32_MAX ||
        (mode != EVK_CAMERA_NEAREST && mode != EVK_CAMERA_SUBPIXEL) || !out_x || !out_y || !keep || (n > 0 && (!x || !y || !map || !map_valid)))
        return EVK_EINVAL;
    // (the rounded coordinates of a kept event are below out_w, out_h: they must fit the output kind)
    if (mode == EVK_CAMERA_NEAREST && out_kind == EVK_SELECT_I16 && (out_h > 32768 || out_w > 32768)) return EVK_EINVAL;
    if (n == 0) return EVK_OK;
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = (unsigned)((n + EVK_BLOCK - 1) / EVK_BLOCK);
    with_time_kind(coord_kind, x, [&](auto *xt) {
        typedef typename std::remove_cv<typename std::remove_pointer<decltype(xt)>::type>::type T;
        k_rectify_lookup<T><<<grid, EVK_BLOCK, 0, s>>>(xt, static_cast<const T *>(y), n, map, static_cast<const uint8_t *>(map_valid), h, w,
                                                      out_h, out_w, mode, out_kind, out_x, out_y, static_cast<uint8_t *>(keep),
                                                      static_cast<uint32_t *>(bad));
    });
    return launch_status();
}

extern "C" int evk_camera_remap(const void *src, int dtype, int64_t planes, int h, int w, const double *map, const void *map_valid,
                                int out_h, int out_w, int interpolation, double fill, void *dst, void *stream) {
    if ((dtype != EVK_CAMERA_U8 && dtype != EVK_CAMERA_F32 && dtype != EVK_CAMERA_F64) || planes < 0 || h < 0 || w < 0 || out_h < 0 ||
        out_w < 0 || (int64_t)h * w > INT32_MAX || (int64_t)out_h * out_w > INT32_MAX ||
        (interpolation != EVK_CAMERA_NEAREST && interpolation != EVK_CAMERA_BILINEAR) || !dst)
        return EVK_EINVAL;
    const int64_t ohw = (int64_t)out_h * out_w;
    if (planes > 0 && ohw > 0 && (!map || !map_valid || ((int64_t)h * w > 0 && !src))) return EVK_EINVAL;
    if (planes == 0 || ohw == 0) return EVK_OK;
    hipStream_t s = (hipStream_t)stream;
    const unsigned grid = (unsigned)((ohw + EVK_BLOCK - 1) / EVK_BLOCK);
    const uint8_t *mv = static_cast<const uint8_t *>(map_valid);
    if (dtype == EVK_CAMERA_U8)
        k_remap_planes<<<grid, EVK_BLOCK, 0, s>>>(static_cast<const uint8_t *>(src), planes, h, w, map, mv, out_h, out_w, interpolation, fill,
                                                  static_cast<uint8_t *>(dst));
    else if (dtype == EVK_CAMERA_F32)
        k_remap_planes<<<grid, EVK_BLOCK, 0, s>>>(static_cast<const float *>(src), planes, h, w, map, mv, out_h, out_w, interpolation, fill,
                                                  static_cast<float *>(dst));
    else
        k_remap_planes<<<grid, EVK_BLOCK, 0, s>>>(static_cast<const double *>(src), planes, h, w, map, mv, out_h, out_w, interpolation, fill,
                                                  static_cast<double *>(dst));
    return launch_status();
}
