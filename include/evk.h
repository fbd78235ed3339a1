/*
 * evk.h -- C ABI of libevk.so: MI355X (gfx950 / CDNA4) kernels for the data-parallel core of
 * TimoStoff/event_utils (event -> image / voxel scatter-add binning, linear-flow contrast maximisation).
 *
 * Boundary rules:
 *   - plain C: pointers, sizes, scalars.  No torch / C++ types.  `stream` is a hipStream_t passed as void*
 *     (NULL = the default stream).  Every entry point only ENQUEUES work on `stream` and returns.
 *   - every pointer is a DEVICE pointer unless the parameter is named host_*.
 *   - the library never allocates or frees caller-visible memory; outputs are ACCUMULATED INTO (the caller zero-
 *     or default-initialises them, as the reference does with its `default` image, image.py:77).
 *   - return value: 0 = ok, <0 = EVK_E* argument error, >0 = hipError_t from the launch.  Never throws / exits.
 *   - data-dependent errors the reference raises as Python exceptions (index out of range: image.py:30-36,96-99) are
 *     counted on the device in `oob` (uint32, caller-zeroed, may be NULL = unchecked); offending events are
 *     dropped; the host wrapper raises the reference's exception type when the counter is non-zero.
 *
 * Reference citations are file:line relative to the reference checkout.
 *
 * The Python binding (event_utils_amd/_lib.py) is derived from the declarations below, and it refuses to import a
 * header it cannot read.  So keep their style:
 *   - one `#define EVK_X <integer>` per constant: a decimal or hex literal, optionally negative, in one pair of
 *     parentheses, or suffixed u, U, l or ll;
 *   - the return type (int, int64_t or const char *) and the name evk_x on the line that starts the declaration, which
 *     may then run over several lines; parameters are pointers, the function-pointer typedefs of this header, or
 *     int, int64_t, uint32_t, uint64_t, float, double.
 */
#ifndef EVK_H
#define EVK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EVK_VERSION 100

#define EVK_OK 0
#define EVK_EINVAL (-1)   /* bad size / null pointer / unsupported parameter            */
#define EVK_ESCRATCH (-2) /* caller-provided scratch too small                           */
#define EVK_EALIGN (-3)   /* pointer not aligned as documented                            */
#define EVK_ECOMM (-4)    /* RCCL not available / collective failed                       */

/* flags for evk_iwe_* */
#define EVK_IWE_ABS_POLARITY 1u /* get_iwe(use_polarity=False): ps = |ps|  (objectives.py:184-185)   */
#define EVK_IWE_GRADIENT 2u     /* also accumulate dIWE/dparams (2 planes) (objectives.py:189-192)    */

int evk_version(void);
const char *evk_error_string(int code);

/* ------------------------------------------------------------------------------------------------------------
 * Event image, nearest pixel
 * ---------------------------------------------------------------------------------------------------------- */

/* events_to_image(..., interpolation=None), numpy path: np.ravel_multi_index + np.bincount on the (H+1, W+1)
 * canvas (image.py:28-38).  canvas[y, x] += w (w == NULL -> 1).  Integer accumulate => bit-exact.
 * Events outside [0,canvas_w) x [0,canvas_h) are counted in *oob (reference: ValueError, image.py:30-36). */
int evk_image_nearest_i32(const int32_t *x, const int32_t *y, const int32_t *w, int64_t n, int canvas_h,
                          int canvas_w, int32_t *canvas, uint32_t *oob, void *stream);

/* Same call site with floating-point weights (np.bincount(weights=ps) accumulates in float64, image.py:37). */
int evk_image_nearest_f64(const int32_t *x, const int32_t *y, const double *w, int64_t n, int canvas_h,
                          int canvas_w, double *canvas, uint32_t *oob, void *stream);

/* events_to_image_torch(..., interpolation=None) (image.py:87-99): coordinates truncated toward zero (.long()),
 * events with x >= clipx or y >= clipy are sent to pixel (0,0) WITH their weight (quirk Q8; pass +inf to disable
 * clipping = clip_out_of_range=False), negative indices wrap as torch's index_put_ does, anything still outside
 * the image is counted in *oob (reference: IndexError). img is (h, w) float32. */
int evk_image_nearest_f32(const float *x, const float *y, const float *w, int64_t n, int h, int wd, float clipx,
                          float clipy, float *img, uint32_t *oob, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Event image, bilinear 4-neighbour splat
 * ---------------------------------------------------------------------------------------------------------- */

/* events_to_image_torch(..., interpolation='bilinear') (image.py:79-86) + interpolate_to_image (image.py:102-115):
 * px=floor(x), dx=x-px, events with x >= clipx or y >= clipy get index (0,0) and weight 0;
 * img[py,px]+=w(1-dx)(1-dy), img[py,px+1]+=w dx(1-dy), img[py+1,px]+=w(1-dx)dy, img[py+1,px+1]+=w dx dy (f32). */
int evk_image_bilinear_f32(const float *x, const float *y, const float *w, int64_t n, int h, int wd, float clipx,
                           float clipy, float *img, uint32_t *oob, void *stream);

/* interpolate_to_image (image.py:102-115) on caller-computed integer pixels px, py (int64, torch .long()) and
 * fractions dx, dy: the four accumulates into img (h, wd).  Negative indices wrap, out-of-range counts in *oob. */
int evk_splat_indexed_f32(const int64_t *px, const int64_t *py, const float *dx, const float *dy, const float *w,
                          int64_t n, int h, int wd, float *img, uint32_t *oob, void *stream);

/* interpolate_to_derivative_img (image.py:117-136): d_img is (C, h, wd), w1 and w2 are (C, n) row-major float32. */
int evk_splat_drv_indexed_f32(const int64_t *px, const int64_t *py, const float *dx, const float *dy,
                              const float *w1, const float *w2, int C, int64_t n, int h, int wd, float *d_img,
                              uint32_t *oob, void *stream);

/* events_to_image_drv (image.py:162-217) for arbitrary per-event Jacobians: float64 inputs are cast to float32
 * BEFORE floor/frac (image.py:179-183), IWE splat as above, and if jx/jy != NULL the derivative splat of
 * interpolate_to_derivative_img (image.py:117-136) into d_img (2, h, wd) with w1 = jx*p*mask, w2 = jy*p*mask
 * (image.py:211-212).  jx, jy are (2, n) row-major float64. */
int evk_image_drv_f64(const double *x, const double *y, const double *p, const double *jx, const double *jy,
                      int64_t n, int h, int wd, float clipx, float clipy, float *img, float *d_img, uint32_t *oob,
                      void *stream);

/* image_to_event_weights (image.py:138-160): out[i] = bilinear interpolation of img (h, wd) float32 at (x[i], y[i])
 * (float64), 0 for events with x >= wd-1 or y >= h-1.  Used by get_iwe(return_per_event_contrast=True)
 * (objectives.py:196-198). */
int evk_image_gather_bilinear_f64(const double *x, const double *y, int64_t n, const float *img, int h, int wd,
                                  double *out, uint32_t *oob, void *stream);
/* the same for a float64 image (upstream takes any numpy array: img[...] * weights promotes to float64 either way) */
int evk_image_gather_bilinear_f64img(const double *x, const double *y, int64_t n, const double *img, int h, int wd,
                                     double *out, uint32_t *oob, void *stream);

/* events_to_timestamp_image[_torch] (image.py:219-353): out4 = (4, h, wd) float32 = [sum of normalised timestamps of
 * positive events, count of positive events, the same two for non-positive events], bilinear splat, accumulated into
 * (the caller initialises the count planes to ONE as upstream does, image.py:269,271).  Normalised timestamp
 * nts = (t - ta)/td (mode 0), (-t + ta)/td (mode 1, timestamp_reverse), t (mode 2), in float32. */
int evk_timestamp_images_f32(const float *x, const float *y, const float *t, const float *p, int64_t n, int h, int wd,
                             float clipx, float clipy, int mode, float ta, float td, float *out4, uint32_t *oob,
                             void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Voxel grid (temporal-bilinear, spatially nearest)
 * ---------------------------------------------------------------------------------------------------------- */

/* events_to_voxel_torch (voxel_grid.py:114-153): t_norm = (t - t_first)/(t_last - t_first)*(B-1) in float32,
 * bin weights p*max(0, 1-|t_norm-b|), one nearest-pixel accumulate per touched bin (image.py:87-95 with
 * clip_out_of_range=False).  ONE pass over the events (each event touches <= 2 bins) instead of the reference's B.
 * vox is (B, h, wd) float32.  t_first / t_last are ts[0] / ts[-1] (the caller reads them; they are also what every
 * rank of an event-sharded run must agree on). */
int evk_voxel_f32(const float *x, const float *y, const float *t, const float *p, int64_t n, float t_first,
                  float t_last, int B, int h, int wd, float *vox, uint32_t *oob, void *stream);
/* the same with t_first = t[0], t_last = t[n-1] read by the kernel itself (voxel_grid.py:133-134 takes them from the same
 * column): a caller whose events are on the device needs no device-to-host transfer before the launch */
int evk_voxel_from_events_f32(const float *x, const float *y, const float *t, const float *p, int64_t n, int B, int h,
                              int wd, float *vox, uint32_t *oob, void *stream);

/* Windowed voxelisation: voxel_grids_fixed_n_torch / voxel_grids_fixed_t_torch (voxel_grid.py:37-80) call
 * events_to_voxel_torch once per window; this builds all nseg grids in ONE launch.  seg = nseg+1 device int64 offsets
 * (window s = events [seg[s], seg[s+1])), each window normalises time with its own first / last event
 * (voxel_grid.py:133-134).  vox is (nseg, B, h, wd) float32, accumulated into.  max_seg_len sizes the grid. */
int evk_voxel_segments_f32(const float *x, const float *y, const float *t, const float *p, const int64_t *seg,
                           int nseg, int64_t max_seg_len, int B, int h, int wd, float *vox, uint32_t *oob,
                           void *stream);

/* events_to_voxel (voxel_grid.py:184-217), numpy path: integer coordinates on the (h+1, wd+1) canvas of
 * events_to_image (x == wd / y == h are legal and cropped away, image.py:17,44), float64 arithmetic and output. */
int evk_voxel_f64(const int32_t *x, const int32_t *y, const double *t, const double *p, int64_t n, double t_first,
                  double t_last, int B, int h, int wd, double *vox, uint32_t *oob, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Contrast maximisation: warp, mask, IWE, blur, objective
 * ---------------------------------------------------------------------------------------------------------- */

/* linvel_warp.warp (warps.py:51-61): dt=t-t0; xo=x-dt*vx; yo=y-dt*vy; if jx/jy != NULL they are (2, n) float64:
 * jx=[-dt; 0], jy=[0; -dt]. */
int evk_warp_linvel_f64(const double *x, const double *y, const double *t, int64_t n, double t0, double vx,
                        double vy, double *xo, double *yo, double *jx, double *jy, void *stream);

/* warp_events_flow_torch (lib/transforms/optic_flow.py:5-46): per-pixel flow field (2, h, wd) float32 sampled bilinearly
 * at every event (grid_sample, align_corners=True, zero padding), xo = x + flow_x(x, y) * (t - t0), same for y. */
int evk_warp_flow_field_f32(const float *x, const float *y, const float *t, int64_t n, const float *flow, int h, int wd,
                            float t0, float *xo, float *yo, void *stream);

/* events_bounds_mask (event_util.py:15-28): mask = !(x<=xmin || x>xmax) * !(y<=ymin || y>ymax) as 0.0/1.0. */
int evk_bounds_mask_f64(const double *x, const double *y, int64_t n, double xmin, double xmax, double ymin,
                        double ymax, double *mask, void *stream);

/* get_iwe (objectives.py:165-199) fused for the linear-flow model: warp at t_ref (= ts[-1], :186) in float64 ->
 * events_bounds_mask(0, bounds_w, 0, bounds_h) (:187) -> multiply by mask (:188-190) -> cast to float32, inner mask
 * x >= canvas_w-1 / y >= canvas_h-1, floor/frac (image.py:179-205) -> IWE splat (image.py:102-115) and, with
 * EVK_IWE_GRADIENT, dIWE splat (image.py:117-136; for this model only w1[0] = w2[1] = -dt*p are non-zero).
 * iwe is (canvas_h, canvas_w) f32, diwe is (2, canvas_h, canvas_w) f32.  Per-event values are bit-identical to the
 * reference's; only the summation order differs.  p_scale multiplies the polarity in float64 before everything
 * else (1.0 normally; 100.0 on the adaptive-lifespan path, objectives.py:225).  Columns are float32 (evk_iwe_linvel_f32, 16 B/event) or float64
 * (evk_iwe_linvel_f64, 32 B/event, exact for arbitrary float64 inputs). */
int evk_iwe_linvel_f32(const float *x, const float *y, const float *t, const float *p, int64_t n, double t_ref,
                       double vx, double vy, double bounds_w, double bounds_h, int canvas_h, int canvas_w,
                       uint32_t flags, double p_scale, float *iwe, float *diwe, void *stream);
int evk_iwe_linvel_f64(const double *x, const double *y, const double *t, const double *p, int64_t n, double t_ref,
                       double vx, double vy, double bounds_w, double bounds_h, int canvas_h, int canvas_w,
                       uint32_t flags, double p_scale, float *iwe, float *diwe, void *stream);

/* Largest blur radius the entries taking host_weights accept (scipy's radius int(4 sigma + 0.5): sigma < 8.125); they
 * return EVK_EINVAL beyond it.  A wider blur goes through evk_gaussian_filter_wide_f32. */
#define EVK_MAX_RADIUS 32

/* scipy.ndimage.gaussian_filter(a, sigma) (objectives.py:233,253), mode='reflect': separable correlation with the
 * symmetric kernel host_weights[0..2*radius] (float64, HOST pointer; computed by the caller exactly as scipy does),
 * filtering axes 0..ndim-1 in order, each pass evaluated in float64 and stored as float32.  ndim is 2 or 3; a 3-D
 * (2, H, W) input is also filtered across its first axis (quirk Q4).  src is not modified; tmp is a scratch array of
 * the same size; the result lands in dst.  src, dst, tmp must be distinct.  0 <= radius <= EVK_MAX_RADIUS. */
int evk_gaussian_filter_f32(const float *src, float *dst, float *tmp, int ndim, const int *host_dims,
                            const double *host_weights, int radius, void *stream);
/* evk_gaussian_filter_f32 for any radius >= 0: the 2*radius+1 weights are a DEVICE array (float64).  Same arithmetic and
 * summation order, so the result is the same float32 bits. */
int evk_gaussian_filter_wide_f32(const float *src, float *dst, float *tmp, int ndim, const int *host_dims,
                                 const double *weights, int radius, void *stream);

/* variance_objective.evaluate_function (objectives.py:234-236): out[0] = mean(img), out[1] = var(img - mean(img))
 * (population variance over all n pixels, float64 accumulation), out[2] = sum(img).
 * scratch: >= evk_reduce_scratch_bytes() bytes. out: 4 doubles on the device. */
int evk_variance_f32(const float *img, int64_t n, double *out, void *scratch, int64_t scratch_bytes, void *stream);

/* variance_objective.evaluate_gradient (objectives.py:256-264): for i in {0,1}
 * out[i] = mean( 2*(iwe - mean(iwe)) * diwe[i] ), out[2] = mean(iwe); the caller negates. diwe is (2, n). */
int evk_variance_grad_f32(const float *iwe, const float *diwe, int64_t n, double *out, void *scratch,
                          int64_t scratch_bytes, void *stream);

/* Fused objective post-pass (one launch + a 1-block finalise; the blurred images are never materialised):
 * evaluate_function (objectives.py:231-236): out as evk_variance_f32 but of gaussian_filter(iwe) (host_weights /
 * radius as in evk_gaussian_filter_f32; radius < 0 = no blur).  Bit-identical to the unfused sequence.
 * Every fused post-pass entry (this one, _grad, _fg, _planes, _rows, stats, gradsums and the tiled one-call evaluations)
 * takes radius <= EVK_MAX_RADIUS and returns EVK_EINVAL above it.  For a wider blur the caller materialises the blurred
 * images with evk_gaussian_filter_wide_f32 (the dIWE as one 3-D filter with EVK_POST_MIX, per channel without) and calls
 * the same entry with radius -1 on them; the Python layer does so. */
int evk_objective_variance_f32(const float *iwe, int h, int w, const double *host_weights, int radius, double *out,
                               void *scratch, int64_t scratch_bytes, void *stream);

#define EVK_POST_MIX 1u      /* scipy's 3-D filter of the (2, H, W) dIWE also mixes the two channels (quirk Q4) */
#define EVK_POST_BLUR_IWE 2u /* use the blurred IWE in the gradient (reference_exact=False); default raw (Q5)    */
#define EVK_POST_VALUE 4u    /* evk_cmax_variance_tiled_f32 with EVK_IWE_GRADIENT: also the function value (out as
                                evk_objective_variance_fg_f32)                                                   */
#define EVK_POST_NONE 8u     /* evk_cmax_variance_tiled_f32: stop after the gather -- iwe_buf holds the raw IWE [, dIWE] of
                                this rank's events, ready for the all-reduce of an event-sharded run; `out` untouched  */
/* evaluate_gradient (objectives.py:252-264): out as evk_variance_grad_f32 with diwe replaced by its blurred version. */
int evk_objective_variance_grad_f32(const float *iwe, const float *diwe, int h, int w, const double *host_weights,
                                    int radius, uint32_t flags, double *out, void *scratch, int64_t scratch_bytes,
                                    void *stream);

/* evaluate_function AND evaluate_gradient of one parameter vector from one IWE / dIWE (what a BFGS line search asks for
 * at every trial point, events_cmax.py:345): out = [g0, g1, mean v, var v] with g as evk_objective_variance_grad_f32
 * (same flags) and v = gaussian_filter(iwe) as evk_objective_variance_f32; values identical to the two separate calls. */
int evk_objective_variance_fg_f32(const float *iwe, const float *diwe, int h, int w, const double *host_weights,
                                  int radius, uint32_t flags, double *out, void *scratch, int64_t scratch_bytes,
                                  void *stream);

/* ---- generic objective reductions: the objectives of objectives.py:266-596 other than the variance one differ only in
 * the scalar they take from the (blurred) IWE -----------------------------------------------------------------------
 * evk_objective_stats_f32: v = gaussian_filter(img) (radius < 0: v = img);
 *   out8 = [mean v, var v, sum v, sum v^2, sum exp(v), sum exp(-p v), count(v > thresh), max v]
 *   (sos :329, soe :373-374, moa :421, isoa :450, sosa :497-498, r1 :584-586; exponentials in float64). */
int evk_objective_stats_f32(const float *img, int h, int w, const double *host_weights, int radius, double p,
                            double thresh, double *out8, void *scratch, int64_t scratch_bytes, void *stream);

#define EVK_G_IDENT 0  /* g(a) = a                                    variance :257, sos :349                        */
#define EVK_G_EXP 1    /* g(a) = exp(a)                               soe :395                                        */
#define EVK_G_STEP 2   /* g(a) = a > gparam ? 1 : 0                   isoa :468-469                                   */
#define EVK_G_EXPNEG 3 /* g(a) = exp((double)(float)(-gparam * a))    sosa :513 (forms -p*iwe in float32 first)       */
/* evk_objective_gradsums_f32: d = gaussian_filter(diwe) (3-D with EVK_POST_MIX), a = iwe or, with EVK_POST_BLUR_IWE,
 * gaussian_filter(iwe);  out8 = [.., .., .., sum g(a), sum d0, sum d1, sum g(a) d0, sum g(a) d1] (out8[0..2] as
 * evk_objective_variance_grad_f32). */
int evk_objective_gradsums_f32(const float *iwe, const float *diwe, int h, int w, const double *host_weights, int radius,
                               uint32_t flags, int gfun, double gparam, double *out8, void *scratch,
                               int64_t scratch_bytes, void *stream);

int64_t evk_reduce_scratch_bytes(void);

/* ------------------------------------------------------------------------------------------------------------
 * Parametric motion models (csrc/evk_warps.hip; DESIGN.md "Rotation and xyztheta warps", "Angular-velocity and
 * planar-flow warps").  dt = t - t0; J(i) = (jacobian_x[i], jacobian_y[i]), (dims, n) float64 as evk_warp_linvel_f64.
 *   EVK_WARP_ROTATION  dims 3, host_params = (cx, cy, omega); (u, v) = (x - cx, y - cy), theta = -omega dt, c = cos,
 *     s = sin: x' = cx + c u - s v, y' = cy + s u + c v;
 *     J(cx) = (1-c, -s), J(cy) = (s, 1-c), J(omega) = (dt (s u + c v), -dt (c u - s v))
 *   EVK_WARP_XYZTHETA  dims 4, host_params = (vx, vy, vz, omega, ox, oy); (u, v) = (x - ox, y - oy):
 *     x' = x - dt (vx + vz u - omega v), y' = y - dt (vy + vz v + omega u);
 *     J(vx) = (-dt, 0), J(vy) = (0, -dt), J(vz) = (-dt u, -dt v), J(omega) = (dt v, -dt u)
 *   EVK_WARP_ANGULAR_VELOCITY  dims 3, host_params = (wx, wy, wz, fx, fy, cx, cy): the camera's body-frame angular velocity
 *     in rad/s (static scene) and the intrinsics K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (no skew, no distortion):
 *     b = ((x - cx)/fx, (y - cy)/fy, 1), theta = (wx, wy, wz) dt, R = exp([theta]x) (Rodrigues),
 *     P = R b, x' = fx P0/P2 + cx, y' = fy P1/P2 + cy;
 *     dP/dw = -R [b]x Jr(theta) dt, Jr(theta) = I - (1-cos a)/a^2 [theta]x + (a - sin a)/a^3 [theta]x^2, a = |theta|
 *     (a series below a = 1e-2; exactly I at theta = 0);
 *     J = [[fx/P2, 0, -fx P0/P2^2], [0, fy/P2, -fy P1/P2^2]] dP/dw.
 *     An event with P2 <= 0 (rotated behind the camera) or a non-finite P warps to x' = y' = NaN (and NaN Jacobians);
 *     the fused IWE drops it in the bounds mask.
 *   EVK_WARP_PLANAR_FLOW  dims 8, host_params = (a1, .., a8, ox, oy); (u, v) = (x - ox, y - oy): the instantaneous
 *     motion field of a planar surface (the linearised homography),
 *     x' = x - dt (a1 + a2 u + a3 v + a7 u^2 + a8 u v), y' = y - dt (a4 + a5 u + a6 v + a7 u v + a8 v^2);
 *     J(a1) = (-dt, 0), J(a2) = (-dt u, 0), J(a3) = (-dt v, 0), J(a4) = (0, -dt), J(a5) = (0, -dt u), J(a6) = (0, -dt v),
 *     J(a7) = (-dt u^2, -dt u v), J(a8) = (-dt u v, -dt v^2).
 * Every entry below takes all four model ids.  host_params is a HOST pointer holding the model's own count of doubles.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_WARP_ROTATION 1
#define EVK_WARP_XYZTHETA 2
#define EVK_WARP_ANGULAR_VELOCITY 3
#define EVK_WARP_PLANAR_FLOW 4
#define EVK_IWE_DIRECT 32u /* evk_iwe_param_*: the direct global-atomic kernel whatever the canvas (EVK_IMPL=direct)     */

/* <model>_warp.warp: xo, yo (n) and, when jx / jy are not NULL, the (dims, n) Jacobians. */
int evk_warp_param_f64(int model, const double *x, const double *y, const double *t, int64_t n, double t0,
                       const double *host_params, double *xo, double *yo, double *jx, double *jy, void *stream);

/* get_iwe fused for these models, as evk_iwe_linvel_*: warp at t_ref in float64 -> events_bounds_mask(0, bounds_w, 0,
 * bounds_h) (Q2) -> p * p_scale [|p| with EVK_IWE_ABS_POLARITY] -> float32, inner clip, floor / fraction -> IWE splat and,
 * with EVK_IWE_GRADIENT, the dIWE splat into dims planes with w1 = float(jx_i) mp, w2 = float(jy_i) mp (image.py:117-136).
 * iwe is (canvas_h, canvas_w), diwe (dims, canvas_h, canvas_w), float32, accumulated into (the caller zeroes them).
 * Canvas rows are accumulated in LDS bands (evk_iwe_param_band_rows rows each) and flushed with global float atomics; a
 * canvas for which that returns 0, or EVK_IWE_DIRECT, takes the direct global-atomic kernel. */
int evk_iwe_param_f32(int model, const float *x, const float *y, const float *t, const float *p, int64_t n, double t_ref,
                      const double *host_params, double bounds_w, double bounds_h, int canvas_h, int canvas_w,
                      uint32_t flags, double p_scale, float *iwe, float *diwe, void *stream);
int evk_iwe_param_f64(int model, const double *x, const double *y, const double *t, const double *p, int64_t n,
                      double t_ref, const double *host_params, double bounds_w, double bounds_h, int canvas_h,
                      int canvas_w, uint32_t flags, double p_scale, float *iwe, float *diwe, void *stream);
/* rows per LDS band of evk_iwe_param_* for this model, flags and canvas; 0 = the direct kernel runs. */
int evk_iwe_param_band_rows(int model, uint32_t flags, int canvas_h, int canvas_w);

/* Gradient sums over 1 <= nplanes <= 8 derivative planes of ALREADY blurred images a (h, w) and d (nplanes, h, w):
 * out = [sum a, sum a^2, sum g(a), sum d_0 .. sum d_{nplanes-1}, sum g(a) d_0 .. sum g(a) d_{nplanes-1}] (3 + 2 nplanes
 * doubles, device), g = EVK_G_*.  Variance gradient: 2/N (sum a d_i - mean(a) sum d_i).  scratch: evk_reduce_scratch_bytes(). */
int evk_objective_gradsums_planes_f32(const float *a, const float *d, int nplanes, int h, int w, int gfun, double gparam,
                                      double *out, void *scratch, int64_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Average-timestamp objective (csrc/evk_tsobj.hip): the loss of Zhu et al., "Unsupervised Event-based
 * Learning of Optical Flow, Depth and Egomotion" (CVPR 2019; upstream objectives.py:524-558, whose
 * events_to_zhu_timestamp_image is undefined), with an analytic gradient.  Definition, for events (x, y, t, p) in stream
 * order, a warp with parameters theta and a canvas (canvas_h, canvas_w) = (H + 1, W + 1):
 *  1. (x', y') = warp(x, y, t - t_ref; theta), float64, the expressions of evk_iwe_param_* / evk_iwe_linvel_*;
 *  2. an event counts when events_bounds_mask(x', y', 0, bounds_w, 0, bounds_h) holds and, after the cast to float32,
 *     x' < canvas_w - 1 and y' < canvas_h - 1 (get_iwe's masks).  A masked event contributes NOTHING, the NaN events of the
 *     angular-velocity model included (upstream's text multiplies the columns by the mask, which would pile every masked
 *     event onto pixel (0, 0): an artefact of the missing function, not kept);
 *  3. tau = (t - t_first) / tdiv with tdiv = t_last - t_first + 1e-6 of the UNWARPED stream (image.py:328), formed by the
 *     caller; float32 arithmetic on float32 columns;
 *  4. per polarity class c (+: p > 0, -: p <= 0): T_c = sum tau w, C_c = sum w over the four bilinear weights w of
 *     (x', y'): the planes out4 = [T+, C+, T-, C-], the order of evk_timestamp_images_f32;
 *  5. A_c = T_c / (1 + C_c): the count images start at ONE upstream (image.py:269,271), which keeps A_c smooth;
 *  6. B_c = gaussian_filter(A_c) per class (radius < 0: B_c = A_c);
 *  7. loss = sum B_+^2 + sum B_-^2, to be MINIMISED (upstream's text returns the negative, which would make every
 *     optimiser drive the events apart: deliberate deviation);
 *  8. gradient by the adjoint: S_c = gaussian_filter(B_c) (the reflect-mode blur with a symmetric kernel is self-adjoint),
 *     gT_c = 2 S_c / (1 + C_c), gC_c = -2 S_c T_c / (1 + C_c)^2,
 *     dloss/dtheta_k = sum_e (tau d_x gT_c + d_x gC_c) Jx_k + (tau d_y gT_c + d_y gC_c) Jy_k, with J the model's Jacobian
 *     (above; linear flow: J(vx) = (-dt, 0), J(vy) = (0, -dt)) cast to float32 once, and d_x g, d_y g the derivatives of
 *     the bilinear interpolant of g at (x', y'): with corners a b / c d and fractions (dx, dy),
 *     d_x g = (b - a)(1 - dy) + (d - c) dy, d_y g = (c - a)(1 - dx) + (d - b) dx.
 * model: EVK_WARP_LINVEL = the linear flow, host_params = (vx, vy), or EVK_WARP_ROTATION .. EVK_WARP_PLANAR_FLOW.  Columns
 * need only the alignment of their elements.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_WARP_LINVEL 0 /* these entries only: evk_warp_param_f64 / evk_iwe_param_* refuse it */
/* steps 1-4: acc4 (4, canvas_h, canvas_w) 64-bit fixed point with 32 fractional bits, accumulated into (the caller zeroes
 * it), then out4 (4, canvas_h, canvas_w) float32 = acc4 2^-32, overwritten.  Integer adds commute: the planes, and the loss
 * and gradient taken from them, are the same bits from call to call.  LDS bands of evk_tsimg_band_rows rows flushed with
 * global 64-bit atomics; the direct global-atomic kernel where that returns 0 and with EVK_IWE_DIRECT in flags. */
int evk_tsimg_warp_f32(int model, const float *x, const float *y, const float *t, const float *p, int64_t n, double t_ref,
                       double t_first, double tdiv, const double *host_params, double bounds_w, double bounds_h,
                       int canvas_h, int canvas_w, uint32_t flags, uint64_t *acc4, float *out4, void *stream);
int evk_tsimg_warp_f64(int model, const double *x, const double *y, const double *t, const double *p, int64_t n,
                       double t_ref, double t_first, double tdiv, const double *host_params, double bounds_w,
                       double bounds_h, int canvas_h, int canvas_w, uint32_t flags, uint64_t *acc4, float *out4,
                       void *stream);
/* rows per LDS band of evk_tsimg_warp_* for these flags and this canvas (four planes); 0 = the direct kernel runs. */
int evk_tsimg_band_rows(uint32_t flags, int canvas_h, int canvas_w);
/* step 5: avg2 = (2, h, w) float32 [A+, A-]. */
int evk_tsimg_average_f32(const float *planes4, int h, int w, float *avg2, void *stream);
/* steps 5-7 and the adjoint images of step 8: out[0] = loss (device double; float64 two-stage reduction in a fixed order);
 * adj4 = (4, h, w) float32 [gT+, gC+, gT-, gC-], or NULL for the value alone.  The blur is evk_gaussian_filter_f32 with
 * host_weights (radius <= EVK_MAX_RADIUS) or evk_gaussian_filter_wide_f32 with dev_weights (above it), class by class;
 * radius < 0: none.  work6: 6 h w floats of scratch; scratch: evk_reduce_scratch_bytes(). */
int evk_tsobj_post_f32(const float *planes4, int h, int w, const double *host_weights, const double *dev_weights,
                       int radius, float *work6, float *adj4, double *out, void *scratch, int64_t scratch_bytes,
                       void *stream);
/* step 8, the adjoint gather: out[0 .. dims) (device doubles) = dloss/dtheta.  One pass over the events, float64 sums
 * reduced per wave, per workgroup and by a final kernel in a fixed order -- no atomics: the same inputs give the same bits.
 * scratch: evk_reduce_scratch_bytes(). */
int evk_tsobj_grad_f32(int model, const float *x, const float *y, const float *t, const float *p, int64_t n, double t_ref,
                       double t_first, double tdiv, const double *host_params, double bounds_w, double bounds_h,
                       int canvas_h, int canvas_w, const float *adj4, double *out, void *scratch, int64_t scratch_bytes,
                       void *stream);
int evk_tsobj_grad_f64(int model, const double *x, const double *y, const double *t, const double *p, int64_t n,
                       double t_ref, double t_first, double tdiv, const double *host_params, double bounds_w,
                       double bounds_h, int canvas_h, int canvas_w, const float *adj4, double *out, void *scratch,
                       int64_t scratch_bytes, void *stream);

/* The same loss as a function of a DENSE flow field (csrc/evk_flowloss.hip; DESIGN.md section 6, "Average-timestamp loss of a
 * flow field"): the unsupervised flow loss of the same paper, with dloss/dflow at every pixel.  Per sample: events (x, y, t, p)
 * in stream order, a field flow (2, h, w) float32, the canvas (h + 1, w + 1).  Steps 2-7 are those above (bounds (0, w] x (0, h]
 * plus the inner clip; a masked event adds nothing; the caller multiplies a polarity factor into p); steps 1 and 8 become
 *  1'. (u, v) = the bilinear sample of flow at (x, y) with zero padding, computed as evk_warp_flow_field_f32 computes it (the
 *      same float32 expressions in the same order, the normalise / denormalise round trip included); x' = x + u dt,
 *      y' = y + v dt in float32, dt = t - t_ref: the bits warp_events_flow_torch returns;
 *  8'. with e_x = tau d_x gT_c + d_x gC_c and e_y likewise (the slopes of step 8 at (x', y'), one-sided by the floor
 *      convention when an event sits on a pixel edge) and b_j the four bilinear weights of (x, y) in the field:
 *      dloss/dflow[0, j] += b_j dt e_x, dloss/dflow[1, j] += b_j dt e_y; corners outside the field, and corners of weight
 *      exactly 0, receive nothing.
 * The kernels see the time constants tc = (t_ref, t_origin, tdiv) float32 per sample, tau = (t - t_origin) / tdiv:
 *   EVK_FLOWTS_FORWARD   t_ref = t_last,  t_origin = t_first, tdiv =   t_last - t_first + 1e-6   (tau = (t - t_first) / tdiv)
 *   EVK_FLOWTS_BACKWARD  t_ref = t_first, t_origin = t_last,  tdiv = -(t_last - t_first + 1e-6)  (tau = (t_last - t) / |tdiv|)
 * in float32 arithmetic on the float32 column; the paper's loss is the sum of the two.  An empty sample has tc = (0, 0, 1e-6),
 * loss 0, zero planes and a zero gradient; a sample of one event has tau = 0.
 * Batches: flow (batch, 2, h, w), the events of all samples concatenated, offsets (batch + 1) int64 on the DEVICE (sample b owns
 * [offsets[b], offsets[b + 1]); the kernels clamp them into [0, n_total]), every per-sample array with a leading batch axis.
 * Columns need only the alignment of their elements.  1 <= batch <= 65535, h >= 2, w >= 2.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_FLOWTS_FORWARD 0
#define EVK_FLOWTS_BACKWARD 1
/* tc (batch, 3) float32, read on the device from offsets and t: no host round trip per sample. */
int evk_flowts_time_constants_f32(const float *t, const int64_t *offsets, int batch, int64_t n_total, int direction, float *tc,
                                  void *stream);
/* steps 1'-4, one pass over the events (grid.y = sample): acc4 (batch, 4, h + 1, w + 1) 64-bit fixed point with 32 fractional
 * bits, accumulated into with global 64-bit integer atomics (the caller zeroes it), then out4 (batch, 4, h + 1, w + 1) float32
 * = acc4 2^-32, overwritten: the contract of evk_tsimg_warp_f32, the direct kernel only (no LDS band form: every band would
 * redo the eight-load field sample). */
int evk_flowts_warp_f32(const float *x, const float *y, const float *t, const float *p, const int64_t *offsets, int batch,
                        int64_t n_total, const float *flow, int h, int w, const float *tc, uint64_t *acc4, float *out4,
                        void *stream);
/* step 8', one pass: re-warp, mask, gather the eight adj4 values of the event's class (adj4 (batch, 4, h + 1, w + 1) from
 * evk_tsobj_post_f32, sample by sample), scatter to the field.  grad (batch, 2, h, w) float32, overwritten, is bitwise
 * repeatable: the terms are summed in 64-bit fixed point in gacc (batch, 2, h, w; the caller zeroes it) at a per-sample scale
 * 2^k taken on the device.  With M = max |adj4| of the sample (absmax: batch words of scratch, reduced here), D = |t_ref -
 * t_origin| >= |dt| and n the sample's events, |term| <= 4 M D, and k = 61 - ilogb(4 M D n), so that n terms cannot leave 63
 * bits.  Quantisation: each term is rounded to 2^-(k+1), 2^-k <= 4 M D n 2^-61, so a cell that m events reach is off by at most
 * m 2^-(k+1) <= m n 2^-62 times the largest possible term 4 M D (2^-22 of it when all of 2^20 events meet in one cell), before
 * the one rounding to float32.  M = 0, D = 0 or n = 0: every term is zero and so is grad; M not finite: grad is NaN. */
int evk_flowts_grad_f32(const float *x, const float *y, const float *t, const float *p, const int64_t *offsets, int batch,
                        int64_t n_total, const float *flow, int h, int w, const float *tc, const float *adj4,
                        uint32_t *absmax, int64_t *gacc, float *grad, void *stream);

/* Contrast (focus) loss of a DENSE flow field (csrc/evk_flowloss.hip; DESIGN.md section 6, "Contrast loss of a flow field"): the
 * loss dense event flow is trained and optimised with (Gallego et al., CVPR 2019; Shiba et al., ECCV 2022; Paredes-Valles et al.,
 * NeurIPS 2021), with dloss/dflow at every pixel.  Per sample: events (x, y, t, p) in stream order, a field flow (2, h, w)
 * float32, the canvas (h + 1, w + 1) with P = (h + 1)(w + 1) pixels; batches, offsets and tc as for the timestamp loss above.
 *  1. warp and mask: steps 1' and 2 above, unchanged (0 < x' < w, 0 < y' < h; x' is bit for bit warp_events_flow_torch's);
 *     t_ref = tc[0]: EVK_FLOWTS_FORWARD is t_last, EVK_FLOWTS_BACKWARD t_first.  An event whose weight is NaN adds nothing;
 *  2. weight: q = p * p_scale, or |p * p_scale| with EVK_FLOWCM_ABS (get_iwe's use_polarity=False), cast to float32 once;
 *  3. IWE: I = sum_e q_e (the four bilinear weights of (x', y')), ONE plane, summed in 64-bit fixed point at a per-sample scale
 *     2^kI taken on the device: with Q = max |q| over the sample's slice (NaN weights left out) and n its event count a cell
 *     receives at most one term per event, each of magnitude <= Q, so |cell| <= Q n < 2^(E + 1), E = ilogb(Q n), and kI = 61 - E
 *     keeps the scaled sum below 2^62 and the n roundings (1/2 each) below 2^62 more: no wrap for any finite p.  Each term is
 *     rounded to 2^-(kI+1) <= Q n 2^-62.  Q n = 0: a zero plane; Q not finite: a NaN plane;
 *  4. blur: B = gaussian_filter(I) (evk_gaussian_filter_f32: reflect, float64 passes stored as float32; radius < 0: B = I);
 *  5. loss, to be MINIMISED (float64 two-stage reductions in a fixed order):
 *       EVK_FLOWCM_VARIANCE     L = -(1/P) sum (B - mean B)^2  (variance_objective.evaluate_function with reference_exact=False;
 *                               the pixel set includes the pad row and column, quirk Q6)
 *       EVK_FLOWCM_MEAN_SQUARE  L = -(1/P) sum B^2             (the sos focus function as a mean);
 *  6. adjoint image G = dL/dI, (h + 1, w + 1) float32: the reflect-mode blur with a symmetric normalised kernel is self-adjoint
 *     and keeps constants, so G = -(2/P) (gaussian_filter(B) - mean B) for the variance and -(2/P) gaussian_filter(B) for the
 *     mean square;
 *  7. field gradient: with e_x, e_y the slopes of the bilinear interpolant of G at (x', y') (step 8's formula, one-sided by the
 *     floor convention) and b_j the four bilinear weights of (x, y) in the field: dL/dflow[0, j] += b_j dt q e_x,
 *     dL/dflow[1, j] += b_j dt q e_y; corners outside the field, and corners of weight exactly 0, receive nothing.  Summed in
 *     64-bit fixed point at a per-sample scale 2^k: with M = max |G|, D = |t_ref - t_origin| >= |dt| and a slope a convex
 *     combination of differences of two values of magnitude <= M, |term| <= 2 M D Q, bound = 2 M D Q n and k = 61 -
 *     ilogb(bound); each term is rounded to 2^-(k+1) <= bound 2^-62.  bound = 0: a zero gradient; not finite: NaN.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_FLOWCM_ABS 1u /* flags of evk_flowcm_warp_f32 / evk_flowcm_grad_f32 */
#define EVK_FLOWCM_VARIANCE 0
#define EVK_FLOWCM_MEAN_SQUARE 1
/* steps 1-3, one pass over the events (grid.y = sample) after the reduction of qmax (batch words: the bit pattern of Q per
 * sample, set here and read again by evk_flowcm_grad_f32): acc (batch, h + 1, w + 1) 64-bit fixed point, accumulated into with
 * global 64-bit integer atomics (the caller zeroes it), then iwe (batch, h + 1, w + 1) float32 = acc 2^-kI, overwritten.  Integer
 * adds commute: the plane, and the loss and gradient taken from it, are the same bits from call to call. */
int evk_flowcm_warp_f32(const float *x, const float *y, const float *t, const float *p, const int64_t *offsets, int batch,
                        int64_t n_total, const float *flow, int h, int w, const float *tc, double p_scale, uint32_t flags,
                        uint32_t *qmax, uint64_t *acc, float *iwe, void *stream);
/* steps 4-6 of ONE sample: iwe and adj are (h, w) float32 planes -- h, w are the CANVAS here, as in evk_tsobj_post_f32, whose
 * conventions for host_weights / dev_weights / radius and scratch this entry shares.  out[0] = L (device double); adj = G, or
 * NULL for the value alone; work: 3 h w floats of scratch. */
int evk_flowcm_post_f32(const float *iwe, int h, int w, const double *host_weights, const double *dev_weights, int radius,
                        int objective, float *work, float *adj, double *out, void *scratch, int64_t scratch_bytes,
                        void *stream);
/* step 7, one pass: the absmax of adj (batch words of scratch, reduced here), re-warp, mask, gather the four values of adj
 * (batch, h + 1, w + 1) around (x', y'), scatter to the field in gacc (batch, 2, h, w; the caller zeroes it), then grad
 * (batch, 2, h, w) float32 = gacc 2^-k, overwritten and bitwise repeatable.  qmax: as evk_flowcm_warp_f32 left it for the same
 * events, p_scale and flags. */
int evk_flowcm_grad_f32(const float *x, const float *y, const float *t, const float *p, const int64_t *offsets, int batch,
                        int64_t n_total, const float *flow, int h, int w, const float *tc, double p_scale, uint32_t flags,
                        const float *adj, const uint32_t *qmax, uint32_t *absmax, int64_t *gacc, float *grad, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Motion segmentation by motion compensation (csrc/evk_segment.hip; DESIGN.md section 6, "Motion segmentation"): the
 * per-cluster weighted images and the soft event assignment of Stoffregen, Gallego, Drummond, Kleeman and Scaramuzza,
 * "Event-Based Motion Segmentation by Motion Compensation" (ICCV 2019).  Inputs: events (x, y, t, p) in stream order; one warp
 * model (EVK_WARP_LINVEL .. EVK_WARP_PLANAR_FLOW, as evk_tsimg_warp_*); L clusters, 1 <= L <= EVK_SEG_MAX_CLUSTERS, with
 * parameters theta_l: host_params is L rows of the model's host_params block (2, 3, 6, 7, 10 doubles per row); associations
 * probs (L, n) float32 on the device, cluster-major, 0 <= P <= 1; the canvas (canvas_h, canvas_w) = (H + 1, W + 1) with
 * Pix = canvas_h canvas_w pixels.
 *  1. warp and mask: per cluster (x'_l, y'_l) = warp(x, y, t - t_ref; theta_l) in float64; mask, cast to float32 and floor /
 *     fraction are those of the average-timestamp objective (steps 1-2 there): an event lands where get_iwe puts it.  An
 *     event may count for some clusters and not for others; a NaN polarity counts for none;
 *  2. weight: q_kl = P_kl, or with EVK_SEG_POLARITY q_kl = s_k P_kl, s_k = +1 for p > 0 and -1 for p <= 0.  |q| <= 1, so the
 *     fixed point of evk_tsimg_warp_* (32 fractional bits) applies with no scale search.  P_kl == 0 or NaN adds nothing;
 *  3. cluster images: I_l = sum_k q_kl (the four bilinear weights of (x'_kl, y'_kl)): L planes summed in 64-bit fixed point
 *     and converted to float32 -- the same bits on every call;
 *  4. B_l = gaussian_filter(I_l); loss, to be MINIMISED: -sum_l Var(B_l); adjoint images G_l = -(2 / Pix)
 *     (gaussian_filter(B_l) - mean B_l): evk_flowcm_post_f32 with EVK_FLOWCM_VARIANCE once per plane, the L values summed by
 *     the caller in cluster order;
 *  5. gradient: dLoss/dtheta_{l,d} = sum_k q_kl (e_x Jx_d + e_y Jy_d), e_x, e_y the one-sided slopes of the bilinear
 *     interpolant of G_l at (x'_kl, y'_kl) (step 8 of the average-timestamp objective), J the model's Jacobian cast to float32
 *     once; float64 sums reduced per wave, per workgroup and by a final kernel in a fixed order: bitwise repeatable;
 *  6. assignment: c_kl = max(0, s_k bilinear(B_l; x'_kl, y'_kl)) where the event counts under theta_l, else 0 (s_k = 1
 *     without EVK_SEG_POLARITY); the four float32 values are combined in float64.  S_k = sum_l c_kl in cluster order.
 *     S_k > 0: P'_kl = (float)(c_kl / S_k); otherwise P'_kl = P_kl (an event no cluster keeps on the canvas keeps its row).
 *     label_k = argmax_l P'_kl, the lowest l on ties.  B_l are the blurred images of step 4, taken with the OLD P.
 * Columns, probs, probs_out and labels need only the alignment of their elements (EVK_EALIGN otherwise); 16-byte loads and
 * stores are used where the addresses allow.  n == 0 is legal: zero planes, a zero gradient, nothing written to probs_out.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_SEG_MAX_CLUSTERS 8
#define EVK_SEG_POLARITY 1u /* flags of evk_seg_*; EVK_IWE_DIRECT is taken too (evk_seg_splat_*: the direct kernel) */
/* steps 1-3: accL (L, canvas_h, canvas_w) 64-bit fixed point with 32 fractional bits, accumulated into (the caller zeroes
 * it), then outL (L, canvas_h, canvas_w) float32 = accL 2^-32, overwritten.  LDS bands of evk_seg_band_rows rows holding all
 * L planes, flushed with global 64-bit atomics; the direct global-atomic kernel where that returns 0 and with EVK_IWE_DIRECT:
 * both give the same bits. */
int evk_seg_splat_f32(int model, const float *x, const float *y, const float *t, const float *p, int64_t n, double t_ref,
                      const double *host_params, int L, const float *probs, double bounds_w, double bounds_h, int canvas_h,
                      int canvas_w, uint32_t flags, uint64_t *accL, float *outL, void *stream);
int evk_seg_splat_f64(int model, const double *x, const double *y, const double *t, const double *p, int64_t n, double t_ref,
                      const double *host_params, int L, const float *probs, double bounds_w, double bounds_h, int canvas_h,
                      int canvas_w, uint32_t flags, uint64_t *accL, float *outL, void *stream);
/* rows per LDS band of evk_seg_splat_* for L clusters, these flags and this canvas; 0 = the direct kernel runs. */
int evk_seg_band_rows(int L, uint32_t flags, int canvas_h, int canvas_w);
/* step 5: out (L, dims) doubles on the device = dLoss/dtheta from adjL (L, canvas_h, canvas_w) float32, the G_l of step 4.
 * One pass over the events per cluster (grid.y = cluster).  scratch: evk_seg_grad_scratch_bytes(). */
int evk_seg_grad_f32(int model, const float *x, const float *y, const float *t, const float *p, int64_t n, double t_ref,
                     const double *host_params, int L, const float *probs, double bounds_w, double bounds_h, int canvas_h,
                     int canvas_w, uint32_t flags, const float *adjL, double *out, void *scratch, int64_t scratch_bytes,
                     void *stream);
int evk_seg_grad_f64(int model, const double *x, const double *y, const double *t, const double *p, int64_t n, double t_ref,
                     const double *host_params, int L, const float *probs, double bounds_w, double bounds_h, int canvas_h,
                     int canvas_w, uint32_t flags, const float *adjL, double *out, void *scratch, int64_t scratch_bytes,
                     void *stream);
int64_t evk_seg_grad_scratch_bytes(void);
/* step 6: blurredL (L, canvas_h, canvas_w) float32 = the B_l; probs_out (L, n) float32 and labels (n) int32, overwritten;
 * probs_out must not be probs. */
int evk_seg_assign_f32(int model, const float *x, const float *y, const float *t, const float *p, int64_t n, double t_ref,
                       const double *host_params, int L, const float *probs, double bounds_w, double bounds_h, int canvas_h,
                       int canvas_w, uint32_t flags, const float *blurredL, float *probs_out, int32_t *labels, void *stream);
int evk_seg_assign_f64(int model, const double *x, const double *y, const double *t, const double *p, int64_t n, double t_ref,
                       const double *host_params, int L, const float *probs, double bounds_w, double bounds_h, int canvas_h,
                       int canvas_w, uint32_t flags, const float *blurredL, float *probs_out, int32_t *labels, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Tile-bucketed path (the fast path).  Global float atomics sustain only ~21 G/s on MI355X, so
 * the hot configurations bucket the events by output tile once and accumulate per tile in LDS.
 * ---------------------------------------------------------------------------------------------------------- */

#define EVK_KEY_NEAREST 0     /* tile of (trunc(x), trunc(y)) with torch's negative wrap; out-of-domain events are
                                 dropped and counted in *oob (voxel_grid.py:140-142 -> image.py:87-99)            */
#define EVK_KEY_FLOOR_CLAMP 1 /* tile of (floor(x), floor(y)) clamped into the domain (IWE: the tile only seeds the
                                 LDS window, every event stays legal)                                             */

/* number of tiles of a (dom_h, dom_w) domain cut into 2^th_log2 x 2^tw_log2 tiles; <0 if unsupported (> 8192). */
int evk_bucket_num_tiles(int dom_h, int dom_w, int tw_log2, int th_log2);
int64_t evk_bucket_scratch_bytes(int ntiles);
/* length (uint32 entries) of the bucket index for n events: tile offsets (ntiles+1), work-item offsets (ntiles+1),
 * per-tile arrival counters (ntiles), the item -> tile map (evk_bucket_max_items entries), the `scene` word and, LAST, the
 * two words of EVK_STAGE_STATS (below); scene = index[len - 3].
 * A tile holding more than max(32768, 4n/ntiles) events is split into several work items, so clustered event data cannot
 * serialise on one CU.  When the fullest tile holds more than 1.25 x the mean tile population the scene word is 1 (a
 * structured scene; 0 otherwise) and the plan is BALANCED: the split threshold is lowered, not below
 * max(4096, 5/8 of the mean), as far as 2 work items per tile allow -- the tile kernels run one workgroup per item, all
 * resident at once, so a launch lasts as long as its largest item. */
int64_t evk_bucket_index_len(int ntiles, int64_t n);
int evk_bucket_max_items(int ntiles, int64_t n);

#define EVK_STAGE_HIST 1    /* per-block tile histograms (reads x, y)                                            */
#define EVK_STAGE_SCAN 2    /* prefix sums -> bucket index                                                       */
#define EVK_STAGE_SCATTER 4 /* write-combining scatter into records (reads x, y, t, p; needs stages 1|2 done)    */
#define EVK_STAGE_ALL 7
#define EVK_STAGE_SHARE_CU 8 /* modifier of the scatter stage: keep its LDS rings <= 96 KB so that workgroups of another,
                                concurrently running kernel (an overlapped RCCL collective) still fit on every CU    */
/* Round 6.  EVK_STAGE_STATS: the histogram pass also reads the polarity column and leaves, in the LAST TWO words of the
 * bucket index, [len - 2] = 0 when every event has a compact 8-byte record (integer pixel coordinates inside the domain, a
 * polarity without low mantissa bits), else 1, and -- filled by the scatter stage (the LDS-sorting one) -- [len - 1] = the
 * float32 bit pattern of max |p| over the bucketed events (0xFFFFFFFF when the ring scatter ran instead): what callers needed a pass over the records
 * (evk_compact_records_f32) and a reduction over p for.  EVK_STAGE_COMPACT (with STATS, IWE key,
 * tiles of <= 1024 pixels): when that verdict is 0 the scatter writes the COMPACT records (see evk_compact_records_f32:
 * same records, same order) into the first 8 n bytes of `records` instead of the 16-byte ones -- the caller learns which
 * from index[len - 2] (also 1 when the tiling forces the ring scatter, which writes 16-byte records only).  EVK_STAGE_LEGACY_SCATTER: the write-combining ring scatter of rounds 1-5 instead of the LDS-sorting
 * one (A/B, tests; both produce identical records). */
#define EVK_STAGE_STATS 16
#define EVK_STAGE_COMPACT 32
#define EVK_STAGE_LEGACY_SCATTER 64

/* Counting sort of the SoA columns by tile: records = n x (x, y, t, p) float4 (16 B, contiguous per tile, time order
 * preserved across the 256 partition blocks), bucket_index = evk_bucket_index_len(ntiles, n) uint32 (see above).
 * Columns and records must be 16-byte aligned (EVK_EALIGN otherwise); n < 2^32.  `stages` = EVK_STAGE_ALL normally;
 * the stages can be launched one by one (same arguments, same scratch) to time them separately. */
int evk_bucket_events_f32(const float *x, const float *y, const float *t, const float *p, int64_t n, int key_mode,
                          int dom_h, int dom_w, int tw_log2, int th_log2, float *records, uint32_t *bucket_index,
                          void *scratch, int64_t scratch_bytes, uint32_t *oob, int stages, void *stream);

/* ---- native on-disk dtypes --------------------------------------------------------------
 * The reference's event files hold xs, ys int16, ts float64, ps bool (HDF5, lib/data_formats/event_packagers.py:90-93)
 * or xy int16 (N, 2), t float64, p uint8 (memmap, lib/data_formats/h5_to_memmap.py:119-121); its loaders widen them on
 * the host (lib/data_loaders/memmap_dataset.py:19-24, hdf5_dataset.py:18-23: float32 coordinates, p * 2.0 - 1.0).
 * These two entry points take the columns as stored -- 13 B/event instead of 16 -- and widen in registers:
 *   x, y      int16; xy_stride 1 = two separate columns, 2 = one interleaved (N, 2) array passed as `x` (y ignored)
 *   t         EVK_T_F64 / EVK_T_F32; the value used is (float)((double)t - t_offset): pass t_offset = ts[0] so that
 *             epoch-scale float64 timestamps survive the narrowing ("t pre-offset by t[0] in f64")
 *   p         EVK_P_U8_PM1: uint8 / bool {0, 1} -> 2p - 1;  EVK_P_U8: uint8 as is;  EVK_P_I8: int8 as is
 * Everything downstream (records, tile kernels) is identical to the float32 path on the widened columns. */
#define EVK_T_F32 0
#define EVK_T_F64 1
#define EVK_P_U8_PM1 0
#define EVK_P_U8 1
#define EVK_P_I8 2
/* (evk_voxel_windows_f32 / evk_pack_window_events_f32 only) float32 polarities, used as they are */
#define EVK_P_F32 3

/* evk_bucket_events_f32 reading native columns (each 16-byte aligned, EVK_EALIGN otherwise). */
int evk_bucket_events_native_f32(const int16_t *x, const int16_t *y, int xy_stride, const void *t, int t_kind,
                                 double t_offset, const void *p, int p_kind, int64_t n, int key_mode, int dom_h,
                                 int dom_w, int tw_log2, int th_log2, float *records, uint32_t *bucket_index,
                                 void *scratch, int64_t scratch_bytes, uint32_t *oob, int stages, void *stream);

/* Native columns -> the four float32 SoA columns every other entry point takes (any alignment); replaces the host
 * casts of memmap_dataset.py:21-23 / hdf5_dataset.py:19-22. */
int evk_native_to_columns_f32(const int16_t *x, const int16_t *y, int xy_stride, const void *t, int t_kind,
                              double t_offset, const void *p, int p_kind, int64_t n, float *out_x, float *out_y,
                              float *out_t, float *out_p, void *stream);

/* events_to_voxel_torch on bucketed records (EVK_KEY_NEAREST over the (h, wd) image; n = the event count that was
 * bucketed): one workgroup per work item, LDS accumulators (B x tile, float64), exclusive plain-store flush: vox += tile,
 * or vox = tile with EVK_VOXEL_OVERWRITE (the caller then needs no memset: every cell is written).  The parts of a
 * split tile meet in `staging` (evk_voxel_tiled_staging_bytes) and the last one to arrive sums them in part order.
 * Same per-event arithmetic as evk_voxel_f32.
 * EVK_VOXEL_SPLIT_POLARITY: events_to_neg_pos_voxel_torch (voxel_grid.py:155-182) in ONE pass instead of two:
 * vox = (2, B, h, wd), [0] = grid of the events with p > 0, [1] = of those with p <= 0, each event with weight 1
 * (2B accumulator planes: pass 2B to evk_voxel_tiled_staging_bytes). */
#define EVK_VOXEL_OVERWRITE 1
#define EVK_VOXEL_SPLIT_POLARITY 2
int64_t evk_voxel_tiled_staging_bytes(int ntiles, int64_t n, int B, int tw_log2, int th_log2);
int evk_voxel_tiled_f32(const float *records, uint32_t *bucket_index, int64_t n, int h, int wd, int tw_log2, int th_log2,
                        float t_first, float t_last, int B, int flags, float *vox, void *staging,
                        int64_t staging_bytes, void *stream);

/* ---- one-pass voxel path (evk_voxel2.hip; DESIGN.md section 3, K1') ---------------------------------------------
 * events_to_voxel_torch (voxel_grid.py:114-153) straight from the event columns in TWO launches: a partition kernel
 * that sorts sub-chunks of <= 16 K events by tile in LDS and writes them back as contiguous runs of 8-byte records
 * (float32 t | 21-bit polarity | pixel in tile; polarities that need more bits go, exactly, to a side array) with a
 * (tile, sub-chunk) table, and a tile kernel that pulls every tile's segments and accumulates in LDS (float64) --
 * the events are read once and written once (24 B/event + the grid instead of 56).  Same per-event arithmetic and
 * results as evk_voxel_f32 / evk_voxel_tiled_f32 -- with one exception: a call all of whose polarities are +1, -1 or +0
 * (and whose accumulators fit, see DESIGN.md K2') is accumulated as an integer count and one int64 fixed-point sum per bin,
 * grid[b] = S0[b] - G[b] + G[b-1], i.e. without rounding p (1 - f) to float32 per event (differences < 6e-8 per event,
 * the parity bar is 1e-5 of the grid's maximum), and such a grid does not depend on the order of the events;
 * EVK_VOXEL2_NO_COUNT keeps the two float64 atomics.
 *   index    evk_voxel2_index_len(ntiles, n) uint32, ZEROED ONCE by the caller when it is allocated; the library
 *            leaves its counters at zero after every call (persistent across calls on one stream)
 *   scratch  evk_voxel2_scratch_bytes(...) bytes, 16-byte aligned, uninitialised
 *   host_report  optional: two uint32, 8-byte aligned, in PINNED host memory the device can write (hipHostMalloc).  As soon as
 *            every partition workgroup has counted the dropped events of its LAST sub-chunk (round 5: ~8 us before the kernel
 *            ends; the bilinear image format: when its last workgroup finishes) the kernel stores {seq, *oob} there (one 8-byte system-scope store: the pair
 *            is never seen torn; EVK_EALIGN if the pointer is not 8-byte aligned), so a caller that checks for
 *            dropped events lazily needs neither a device-to-host copy nor an event on the stream: the call numbered
 *            `seq` has counted all its events once host_report[0] == seq (sequence numbers grow by one per call).
 *            Independent of `oob`: without a counter the report is {seq, 0}.
 *   flags    EVK_VOXEL_OVERWRITE, EVK_VOXEL_SPLIT_POLARITY as evk_voxel_tiled_f32;
 *            EVK_VOXEL_T_FROM_EVENTS: t_first / t_last are read on the device from t[0] / t[n-1] (voxel_grid.py:133-134
 *            takes them from the same column), so the caller needs no device-to-host transfer before the launch;
 *            EVK_VOXEL2_PARTITION_ONLY / EVK_VOXEL2_TILES_ONLY: launch one of the two kernels (timing).
 *            EVK_VOXEL_DETERMINISTIC: the tile kernel accumulates int64 multiples of 2^-32 instead of float64 (integer
 *            adds commute: the grid is bit-identical from run to run and for any order of the events); a NaN t_norm
 *            (t_last == t_first, Q9) marks its cell NaN in every bin as in the reference; every other contribution must be
 *            finite and below 2^30, anything else is counted in index[4] (the caller reads and clears it) and left out.
 * Tiles: tile_w x tile_h PIXELS, any size with (tile_w | 1) * tile_h <= 1024 (evk_voxel2_num_tiles() > 0), at most
 * evk_voxel2_max_tiles() of them.  The tile kernel runs one workgroup per tile, all resident at once, so a tile COUNT
 * that is a multiple of the 256 CUs (640x480: 512 tiles of 20x30) keeps every CU equally busy. */
#define EVK_VOXEL_T_FROM_EVENTS 4
#define EVK_VOXEL_DETERMINISTIC 256
#define EVK_VOXEL2_PARTITION_ONLY 16
#define EVK_VOXEL2_TILES_ONLY 32
#define EVK_VOXEL2_SHARE_CU 128    /* partition with 64 KB of LDS per CU instead of 128 KB, so that workgroups of another,
                                      concurrently running kernel (an overlapped RCCL collective) still fit on every CU */
#define EVK_VOXEL2_NO_XCD_ORDER 64 /* A/B switch: tile kernel work items in plain order instead of one contiguous range per XCD */
/* The library picks the record size (4 bytes above 16 M events, else 8), the unit-polarity counting mode and the tile
 * workgroup size (768 threads where two such workgroups fit a CU) by itself; these flags force the other choice so that tests
 * and measurements can run every shipped kernel shape at any size (results are the same within the parity bar). */
#define EVK_VOXEL2_REC4 1024
#define EVK_VOXEL2_REC8 2048
#define EVK_VOXEL2_NO_COUNT 4096
#define EVK_VOXEL2_WG512 8192
#define EVK_VOXEL2_NO_COUNT2 32768   /* (A/B, tests) where the counting mode's planes do not fit (1280x720 tiles) unit polarities are
                                        still counted in integers, two int64 LDS atomics per event in the float64 mode's planes
                                        (same bits as the counting mode); this flag keeps the float64 atomics there */
/* EVK_VOXEL2_LIVE (round 5): the tiles are accumulated WHILE the partition sorts -- a consumer kernel on a second stream of the
 * library's own (one per device, created on first use) takes every run as soon as it is written, two tiles per workgroup, one
 * workgroup beside the partition's on every CU; the tile kernel proper still follows on `stream` and accumulates only what
 * the consumers leave (polarities other than +1 / -1 / +0, hot tiles, rounds that did not arrive in time), so the call is
 * complete in `stream`'s order exactly as without the flag (round 6: `stream` also WAITS for the consumer kernel's end behind
 * the tile kernel -- an event on the side stream -- so index / scratch / the columns may be freed or rewritten by anything
 * ordered after the call on `stream`, as for every other entry point), and the grid is bit-identical to the counting mode's.  A request:
 * calls the consumer kernel is not written for (more than 512 tiles, accumulators beyond 52 KB per pair of tiles, fewer than
 * two sub-chunks per partition workgroup, 4-byte records, split polarities, EVK_VOXEL2_SHARE_CU, single stages, a stream that
 * is being captured into a graph) run as without it.  evk_voxel2_f32 only. */
#define EVK_VOXEL2_LIVE 16384
/* EVK_COLUMNS_UNALIGNED (round 6; evk_voxel2_f32, evk_image2_nearest_f32 / _bilinear_f32, evk_image2_splat_indexed_f32,
 * evk_image2_splat_drv_indexed_f32 (pixels and fractions), evk_timestamp_images2_f32): the event columns need only the alignment of their elements (4 bytes; 8 for int64 pixels) instead
 * of 16 bytes -- a device SLICE xs[a:b] of a resident stream is read where it lies.  The kernels load 16 bytes at a time and a
 * group of four events that is only partly inside the stream is loaded whole: the caller guarantees that the 12 bytes (24 for
 * int64) behind every column's last event are readable (inside the same allocation).  Without the flag a column that is not
 * 16-byte aligned is refused with EVK_EALIGN, as before. */
#define EVK_COLUMNS_UNALIGNED 65536
int evk_voxel2_max_tiles(void);
int64_t evk_voxel2_index_len(int ntiles, int64_t n);
int evk_voxel2_num_tiles(int h, int wd, int tile_w, int tile_h);   /* 0 = this tiling is not supported */
/* 1 when evk_voxel2_f32 takes this tiling with `planes` accumulator planes (B; 2 B with EVK_VOXEL_SPLIT_POLARITY; 1 for the
 * event images): grid, partition LDS, tile-kernel LDS and tile count all fit.  evk_num_cu(): the CU count the tile count
 * should be a multiple of (256 on MI355X). */
int evk_voxel2_fits(int h, int wd, int tile_w, int tile_h, int planes);
int evk_num_cu(void);
int64_t evk_voxel2_scratch_bytes(int ntiles, int64_t n, int planes, int tile_w, int tile_h);
int evk_voxel2_f32(const float *x, const float *y, const float *t, const float *p, int64_t n, int h, int wd,
                   int tile_w, int tile_h, float t_first, float t_last, int B, int flags, float *vox,
                   uint32_t *index, void *scratch, int64_t scratch_bytes, uint32_t *oob, uint32_t *host_report,
                   uint32_t seq, void *stream);
/* ROW BANDS for event-sharded runs: after an evk_voxel2_f32 call with EVK_VOXEL2_PARTITION_ONLY (same n, h,
 * wd, tile size, B, flags, index, scratch), accumulate only the tile rows [tile_row_lo, tile_row_hi) and WRITE them to `band`,
 * a contiguous (B, rows, wd) float32 buffer (rows = min(tile_row_hi * tile_h, h) - tile_row_lo * tile_h; 2B planes with
 * EVK_VOXEL_SPLIT_POLARITY).  A sharded caller launches the bands one after the other and all-reduces band k (one contiguous
 * buffer) while band k + 1 is being accumulated; event_utils_amd/distributed.py does. */
int evk_voxel2_band_f32(int64_t n, int h, int wd, int tile_w, int tile_h, int B, int flags, int tile_row_lo, int tile_row_hi,
                        float *band, uint32_t *index, void *scratch, int64_t scratch_bytes, void *stream);
/* out[i] = (t[i] - t_first) / (t_last - t_first) * (B - 1) in float32: the normalised time of voxel_grid.py:134, by the very
 * function the partition kernel calls -- bit-identical to numpy's float32 arithmetic; the tests compare it bit for bit. */
int evk_normalise_time_f32(const float *t, int64_t n, float t_first, float t_last, int B, float *out, void *stream);
/* the same from the reference's on-disk dtypes (see evk_bucket_events_native_f32) */
int evk_voxel2_native_f32(const int16_t *x, const int16_t *y, int xy_stride, const void *t, int t_kind, double t_offset,
                          const void *p, int p_kind, int64_t n, int h, int wd, int tile_w, int tile_h, float t_first,
                          float t_last, int B, int flags, float *vox, uint32_t *index, void *scratch,
                          int64_t scratch_bytes, uint32_t *oob, uint32_t *host_report, uint32_t seq, void *stream);

/* ---- event images on the one-pass partition (evk_image2.hip) -------------------------------
 * The three event-image entry points above (evk_image_nearest_i32 / _f32, evk_image_bilinear_f32: one global atomic per
 * contribution, ~21 G atomics/s) on the voxel grid's partition + LDS-tile design: the same results -- the integer image
 * bit for bit, the float32 images up to the order of the additions -- from two launches that read 12 B/event and move a
 * 4-byte (nearest) or 12-byte (bilinear) record once.  Semantics, clip thresholds, the treatment of negative /
 * out-of-range / non-finite coordinates and the meaning of *oob are those of the corresponding direct entry point
 * (the partition kernel hands the events an LDS tile cannot take to the direct kernel's own code).
 *   tile_w, tile_h   as evk_voxel2_f32 (evk_voxel2_num_tiles(h, wd, tile_w, tile_h) > 0)
 *   index            evk_voxel2_index_len(ntiles, n) uint32, zeroed once by the caller, persistent (as evk_voxel2_f32;
 *                    the two paths may share one index on a stream)
 *   scratch          evk_image2_scratch_bytes(ntiles, n, tile_w, tile_h) bytes, 16-byte aligned
 *   host_report/seq  as evk_voxel2_f32
 *   flags            EVK_VOXEL_OVERWRITE (nearest only): every pixel of the image is WRITTEN, the caller needs no memset;
 *                    without it the result is added to the image (the reference's `default` image, image.py:77).  The
 *                    bilinear call always adds.  EVK_VOXEL2_PARTITION_ONLY / _TILES_ONLY / _NO_XCD_ORDER as evk_voxel2_f32.
 *                    EVK_IMAGE2_NO_FIXED: bilinear windows in float64 even when every weight is +1, -1 or +0 (A/B).
 * Columns 16-byte aligned (EVK_EALIGN otherwise).  evk_image2_nearest_i32: w == NULL counts the events (weight 1). */
#define EVK_IMAGE2_NO_FIXED 512
int64_t evk_image2_scratch_bytes(int ntiles, int64_t n, int tile_w, int tile_h);
int evk_image2_nearest_i32(const int32_t *x, const int32_t *y, const int32_t *w, int64_t n, int canvas_h, int canvas_w,
                           int tile_w, int tile_h, int flags, int32_t *canvas, uint32_t *index, void *scratch,
                           int64_t scratch_bytes, uint32_t *oob, uint32_t *host_report, uint32_t seq, void *stream);
int evk_image2_nearest_f32(const float *x, const float *y, const float *w, int64_t n, int h, int wd, float clipx,
                           float clipy, int tile_w, int tile_h, int flags, float *img, uint32_t *index, void *scratch,
                           int64_t scratch_bytes, uint32_t *oob, uint32_t *host_report, uint32_t seq, void *stream);
int evk_image2_bilinear_f32(const float *x, const float *y, const float *w, int64_t n, int h, int wd, float clipx,
                            float clipy, int tile_w, int tile_h, int flags, float *img, uint32_t *index, void *scratch,
                            int64_t scratch_bytes, uint32_t *oob, uint32_t *host_report, uint32_t seq, void *stream);
/* evk_splat_indexed_f32 (above; interpolate_to_image on caller-computed pixels and fractions, image.py:102-115) on the same design
 * (round 6): an event whose px + dx, py + dy are float32 values with floor() == px, py -- every event whose pixel and fraction
 * were taken from a float32 coordinate, as upstream's callers do -- travels as a bilinear record; any other (a sum that rounds,
 * fractions outside [0, 1), NaN, pixels that wrap or raise) is re-read by its index and takes the direct kernel's code inside
 * the partition kernel.  Same arguments and *oob as evk_splat_indexed_f32, the rest as evk_image2_bilinear_f32 (always adds). */
int evk_image2_splat_indexed_f32(const int64_t *px, const int64_t *py, const float *dx, const float *dy, const float *w, int64_t n,
                                 int h, int wd, int tile_w, int tile_h, int flags, float *img, uint32_t *index, void *scratch,
                                 int64_t scratch_bytes, uint32_t *oob, uint32_t *host_report, uint32_t seq, void *stream);
/* The derivative splats on the same design (round 6): evk_splat_drv_indexed_f32 (interpolate_to_derivative_img, image.py:117-136;
 * two channels) and evk_image_drv_f64 (events_to_image_drv, image.py:162-217).  An event's record carries its coordinates
 * relative to the tile and its INDEX in the stream; the tile kernel fetches the event's four or five weights from the caller's
 * columns by that index (they do not fit the partition's LDS) and accumulates the image and / or its two derivative planes in LDS
 * windows.  Arguments and *oob as the direct entry points', the rest as evk_image2_bilinear_f32 (always add; n < 2^32);
 * evk_image2_drv_f64: x, y 16-byte aligned, jx == jy == NULL for the image alone.  `scratch` of these two and of
 * evk_image2_splat_indexed_f32: evk_image2_indexed_scratch_bytes (8 K-event sub-chunks whatever the tile count). */
int64_t evk_image2_indexed_scratch_bytes(int ntiles, int64_t n, int tile_w, int tile_h);
int evk_image2_splat_drv_indexed_f32(const int64_t *px, const int64_t *py, const float *dx, const float *dy, const float *w1,
                                     const float *w2, int64_t n, int h, int wd, int tile_w, int tile_h, int flags, float *d_img,
                                     uint32_t *index, void *scratch, int64_t scratch_bytes, uint32_t *oob, uint32_t *host_report,
                                     uint32_t seq, void *stream);
int evk_image2_drv_f64(const double *x, const double *y, const double *p, const double *jx, const double *jy, int64_t n, int h,
                       int wd, float clipx, float clipy, int tile_w, int tile_h, int flags, float *img, float *d_img,
                       uint32_t *index, void *scratch, int64_t scratch_bytes, uint32_t *oob, uint32_t *host_report, uint32_t seq,
                       void *stream);
/* evk_timestamp_images_f32 (above; events_to_timestamp_image[_torch], image.py:219-353: eight global atomics per event) on
 * the same design (round 6): one partition -- 16 B/event read, a 12-byte record {x, y relative to the tile; the event's
 * class in their sign bits; its normalised time stamp} moved once -- and a tile kernel with four LDS windows per tile
 * (time / count of the positive and of the non-positive events).  Arguments x .. td and the meaning of *oob as
 * evk_timestamp_images_f32, including the upstream quirk (a clipped event lands on pixel (0, 0) with its weights intact);
 * the rest as evk_image2_bilinear_f32, with evk_timestamp_images2_scratch_bytes for `scratch`.  out4 = (4, h, wd), ADDED to. */
int64_t evk_timestamp_images2_scratch_bytes(int ntiles, int64_t n, int tile_w, int tile_h);
int evk_timestamp_images2_f32(const float *x, const float *y, const float *t, const float *p, int64_t n, int h, int wd,
                              float clipx, float clipy, int mode, float ta, float td, int tile_w, int tile_h, int flags,
                              float *out4, uint32_t *index, void *scratch, int64_t scratch_bytes, uint32_t *oob,
                              uint32_t *host_report, uint32_t seq, void *stream);

/* get_iwe (linear flow) on bucketed records (EVK_KEY_FLOOR_CLAMP over a (dom_h, dom_w) domain covering the events):
 * one workgroup per (work item, time slice) accumulates a (win_h x win_w) LDS window (tile + flow halo, origin shifted
 * by the slice's displacement), stores it to `staging`; a gather kernel adds the windows covering each canvas pixel to
 * iwe / diwe.  Events falling outside their window use a global atomic (correct for any flow; slices / win_* only
 * tune speed).  t_first = earliest event time (bounds the window shifts).  Same per-event arithmetic as
 * evk_iwe_linvel_f32.
 * p_bound / dt_bound: upper bounds of |p * p_scale| and of |t - t_ref| over the events (0 / negative = unknown).  With
 * bounds the LDS windows accumulate in FIXED POINT -- this kernel is LDS-atomic bound, ds_add_u64 is 1.5x faster than
 * ds_add_f64 on gfx950, and integer sums are order-independent (bit-reproducible):
 *   - 64-bit cells, value * 2^k with k = min(40, 61 - ceil(log2(n * p_bound * max(1, dt_bound)))), used when k >= 26;
 * Quantisation <= 2^-(k+1) per contribution for the 64-bit cells.  Without bounds: float64 accumulation. */
/* COMPACT RECORDS.  The evaluation kernels stream the bucketed records once per evaluation, and an optimisation evaluates
 * ~10^2 times, so the record stream is what the function evaluation is bound by.  Sensor events have integer pixel
 * coordinates and +-1 polarities: evk_compact_records_f32 rewrites the (x, y, t, p) float32 records of a bucketing
 * (EVK_KEY_FLOOR_CLAMP, tiles of <= 1024 pixels) as 8-byte records {t, polarity bits [31:11] | pixel in tile [9:0]} in the
 * same order, and ORs 1 into *not_compact if some record does not survive that exactly (non-integer or out-of-domain
 * x / y, a polarity with any of its low 11 mantissa bits set).  When *not_compact stays 0 the tiled IWE entry points take
 * the compact buffer as `records` with EVK_IWE_COMPACT in `flags`: x, y are rebuilt from the tile origin, every
 * result is bit-identical to the 16-byte records'.  `compact` holds evk_compact_records_bytes(n) bytes, 16-byte aligned. */
#define EVK_IWE_COMPACT 16u
int64_t evk_compact_records_bytes(int64_t n);
int evk_compact_records_f32(const float *records, int64_t n, int dom_h, int dom_w, int tw_log2, int th_log2,
                            void *compact, uint32_t *not_compact, void *stream);
int64_t evk_iwe_tiled_staging_bytes(int ntiles, int64_t n, int slices, int planes, int win_w, int win_h);
int evk_iwe_linvel_tiled_f32(const float *records, const uint32_t *bucket_index, int64_t n, int dom_h, int dom_w,
                             int tw_log2, int th_log2, int slices, int win_w, int win_h, double t_first, double t_ref,
                             double vx, double vy, double bounds_w, double bounds_h, int canvas_h, int canvas_w,
                             uint32_t flags, double p_scale, double p_bound, double dt_bound, void *staging, int64_t staging_bytes,
                             float *iwe, float *diwe, void *stream);

/* variance_objective.evaluate_function / evaluate_gradient (objectives.py:211-264) in ONE call on bucketed records:
 * memset(iwe_buf) -> evk_iwe_linvel_tiled_f32 -> evk_objective_variance[_grad]_f32.  iwe_buf is (1, ch, cw) or, with
 * EVK_IWE_GRADIENT, (3, ch, cw) float32 = IWE followed by the two dIWE planes (left filled, un-blurred).
 * out: as evk_objective_variance_f32 / evk_objective_variance_grad_f32 / (post_flags & EVK_POST_VALUE)
 * evk_objective_variance_fg_f32.
 * spill_pair (optional): 2 x (1 | 3, ch, cw) float32, ZEROED ONCE by the caller and kept between calls, with `parity`
 * alternating 0 / 1 from call to call on one stream.  The evaluation then needs no memset: the rare events outside their
 * LDS window go to spill[parity], the gather writes iwe_buf = spill[parity] + windows and zeroes what the previous call
 * left in spill[parity ^ 1].
 * host_out (optional, HOST pointer to 4 doubles): the call also delivers `out` there and returns only when it has
 * (the finalise kernel stores the results and a sequence number in a pinned slot that the call polls: no copy command, no
 * stream synchronisation).  Everything enqueued on the stream before the call has completed when it returns. */
int evk_cmax_variance_tiled_f32(const float *records, const uint32_t *bucket_index, int64_t n, int dom_h, int dom_w,
                                int tw_log2, int th_log2, int slices, int win_w, int win_h, double t_first, double t_ref, double vx,
                                double vy, double bounds_w, double bounds_h, int canvas_h, int canvas_w,
                                uint32_t iwe_flags, double p_scale, double p_bound, double dt_bound, const double *host_weights,
                                int radius, uint32_t post_flags, void *staging, int64_t staging_bytes, float *iwe_buf,
                                double *out, void *scratch, int64_t scratch_bytes, float *spill_pair, int parity,
                                double *host_out, void *stream);

/* ---- batched evaluation: three NEARBY flows in one pass over the events ----------------
 * The reference's default optimiser path (numeric_grads=True, events_cmax.py:343) lets scipy estimate the gradient by
 * forward differences with epsilon = 1: f(v), f(v + e1), f(v + e2) = three full get_iwe passes.  These entry points
 * read every event once and accumulate the three IWEs side by side (iwe3 = (3, ch, cw)); host_vx / host_vy are 3
 * doubles each (host pointers).  The flows must be close (they share one LDS window per workgroup; an event outside it
 * still lands through a global atomic, so distant flows are merely slower). */
int evk_iwe_linvel_tiled_batch3_f32(const float *records, const uint32_t *bucket_index, int64_t n, int dom_h, int dom_w,
                                    int tw_log2, int th_log2, int slices, int win_w, int win_h, double t_first,
                                    double t_ref, const double *host_vx, const double *host_vy, double bounds_w,
                                    double bounds_h, int canvas_h, int canvas_w, uint32_t flags, double p_scale,
                                    double p_bound, double dt_bound, void *staging, int64_t staging_bytes, float *iwe3,
                                    void *stream);
/* evk_objective_variance_f32 for nplanes stacked images: out = nplanes x 4 doubles. */
int evk_objective_variance_planes_f32(const float *imgs, int nplanes, int h, int w, const double *host_weights,
                                      int radius, double *out, void *scratch, int64_t scratch_bytes, void *stream);

/* Row-sharded post-pass (multi-GPU option).  img = (1 | 3, hb, w) float32: the rows of ONE row block of the (ch, cw)
 * image -- plane 0 the IWE, planes 1, 2 the dIWE for mode 1 / 3 -- including `radius` halo rows on every side that is not
 * an edge of the whole image, already summed over the ranks.  The block is blurred with the 'reflect' rule at its own
 * edges (exact: an edge of the buffer is either an edge of the image or lies beyond the halo) and the pixels of rows
 * [y_lo, y_hi) of the buffer are added up.  mode 0: sums = [S v, S v^2]; mode 1: [S a, S d0, S d1, S a d0, S a d1];
 * mode 3: those five, then S v, S v^2 of the blurred IWE (flags as evk_objective_variance_grad_f32).  `sums` = 8 doubles
 * (device); all-reduce them over the ranks and finalise: mean = S0 / N, var = S1 / N - mean^2,
 * g_i = 2 / N (S(3+i) - (S0 / N) S(1+i)) with N = ch * cw. */
int evk_objective_variance_rows_f32(const float *img, int mode, int hb, int w, int y_lo, int y_hi,
                                    const double *host_weights, int radius, uint32_t flags, double *sums, void *scratch,
                                    int64_t scratch_bytes, void *stream);
/* memset -> batch3 IWE -> gather -> fused blur + variance of each plane: out12 = 3 x 4 doubles. */
int evk_cmax_variance_batch3_tiled_f32(const float *records, const uint32_t *bucket_index, int64_t n, int dom_h,
                                       int dom_w, int tw_log2, int th_log2, int slices, int win_w, int win_h,
                                       double t_first, double t_ref, const double *host_vx, const double *host_vy,
                                       double bounds_w, double bounds_h, int canvas_h, int canvas_w, uint32_t iwe_flags,
                                       double p_scale, double p_bound, double dt_bound, const double *host_weights, int radius,
                                       void *staging, int64_t staging_bytes, float *iwe3, double *out12, void *scratch,
                                       int64_t scratch_bytes, float *spill_pair, int parity, double *host_out,
                                       void *stream);

/* ---- the whole optimisation in one call (round 6; evk_optim.hip) -------------------------------------------------
 * optimize_contrast for the linear-flow warp and the variance objective (events_cmax.py:313-346, where scipy's fmin_bfgs
 * drives one Python callback per evaluation): the quasi-Newton iteration of event_utils_amd.contrast_max.evk_bfgs with its
 * arithmetic, the LDS window of every pass and the result poll inside the library.  Every pass is one
 * evk_cmax_variance_tiled_f32 (value + gradient at one flow; EVK_POST_VALUE is added to post_flags) or one
 * evk_cmax_variance_batch3_tiled_f32 (three step lengths of the line search); the arguments up to `spill_pair` mean what
 * they mean there (iwe_flags WITHOUT EVK_IWE_GRADIENT; iwe_buf: 3 planes; out12: 12 doubles, device; spill_pair required).
 * Time slices and window are chosen per pass from the flow; `staging_bytes` is the capacity the loop may use
 * (evk_iwe_tiled_staging_bytes of the largest plan the caller wants it to take).
 * parity (host, in/out): the spill parity of the LAST successful evaluation on this pair; updated.
 * x0: 2 doubles.  opts: 6 doubles [xtol (px/s), gtol, ftol, maxiter, numeric_grads (0 | 1: forward differences with
 * epsilon = 1 from one three-flow pass, the reference's default), unit_first (0 | 1)].
 * result (host): 6 + 5 * trace_cap doubles: [x0, x1, f(x), accepted points, event passes, status], then one row
 * [x0, x1, f, g0, g1] per accepted point (the first trace_cap of them).  status 0: finished (converged or maxiter);
 * 1: a trial flow needs a plan this call cannot take (more than 64 time slices, more than 128 candidate windows, more
 * staging than staging_bytes, a non-finite flow) -- x is the last accepted point, the caller continues with its own loop.
 * Returns when the last pass has delivered its results (synchronous, like the evaluation calls with host_out). */
int evk_cmax_bfgs_variance_tiled_f32(const float *records, const uint32_t *bucket_index, int64_t n, int dom_h, int dom_w,
                                     int tw_log2, int th_log2, double t_first, double t_ref, double bounds_w, double bounds_h,
                                     int canvas_h, int canvas_w, uint32_t iwe_flags, double p_scale, double p_bound,
                                     double dt_bound, const double *host_weights, int radius, uint32_t post_flags,
                                     void *staging, int64_t staging_bytes, float *iwe_buf, double *out12, void *scratch,
                                     int64_t scratch_bytes, float *spill_pair, int *parity, const double *x0,
                                     const double *opts, double *result, int trace_cap, void *stream);
/* The same iteration on an evaluator of the caller's (any two-parameter objective; no GPU work of its own -- a host function):
 * fg(user, x[2], &f, g[2]) = value and gradient at x; f3(user, pts[6] = {x0a, x1a, x0b, x1b, x0c, x1c}, fs[3]) = the values at
 * three points (one pass over the events when the objective can do that).  Both return 0, or 1 to decline the point (the
 * run ends with status 1, as above), or any other code, which is returned as it is.  fg may be NULL when opts[4]
 * (numeric_grads) is set: value and gradient then come from f3 at x, x + e0, x + e1.  opts / result / trace_cap as above. */
typedef int (*evk_bfgs2_fg_fn)(void *user, const double *x, double *f, double *g);
typedef int (*evk_bfgs2_f3_fn)(void *user, const double *pts, double *fs);
int evk_bfgs2_minimize(evk_bfgs2_fg_fn fg, evk_bfgs2_f3_fn f3, void *user, const double *x0, const double *opts,
                       double *result, int trace_cap);

/* Largest singular value SQUARED of a float32 (h, w) image, float64 -> out[0]: what the "rms" objective needs
 * (objectives.py:282: np.linalg.norm(iwe, 2) of a 2-D array is the spectral norm).  Lanczos on the Gram operator with full
 * re-orthogonalisation in one workgroup, then a bisection; h, w <= 4096.  scratch: evk_spectral_scratch_bytes(h, w).
 * Round 6: `out` holds TWO doubles.  The Ritz pair's true residual is measured after every sweep of <= 96 steps and the
 * iteration restarts from the Ritz vector until it is below 1e-10 of the value (at most 8 sweeps); out[1] = the final relative
 * residual, a bound on the relative distance of out[0] (a lower bound of sigma_max^2) from an eigenvalue -- a caller that needs
 * more than that checks it. */
int64_t evk_spectral_scratch_bytes(int h, int w);
int evk_spectral_norm_sq_f32(const float *img, int h, int w, double *out, void *scratch, int64_t scratch_bytes, void *stream);

/* ---- the stateful image classes of image.py:355-396 (float64 images, as the reference's numpy arrays) ----------
 * TimestampImage.add_events (image.py:366-368): image[int(y), int(x)] = t per event IN STREAM ORDER -- for every pixel the
 * LAST event that hits it wins.  int() truncates toward zero, a negative index wraps once (numpy indexing), anything else
 * (also NaN / infinity) is counted in *oob (the reference raises IndexError).  last_scratch: h * w uint32, any content.
 * n < 2^32 - 1. */
int evk_timestamp_image_add_f64(const double *x, const double *y, const double *t, int64_t n, int h, int w, double *image,
                                uint32_t *last_scratch, uint32_t *oob, void *stream);
/* EventImage.add_event (image.py:384-385): image[int(y), int(x)] += p.  p == NULL: the indices are only checked -- what
 * upstream's add_events does, which passes a literal 0 for the polarity (image.py:387-389). */
int evk_event_image_add_f64(const double *x, const double *y, const double *p, int64_t n, int h, int w, double *image,
                            uint32_t *oob, void *stream);
/* TimestampImage.get_image (image.py:370-375): out = (scipy.stats.rankdata(image, method='dense') - 1) / its maximum
 * (0 / 0 = NaN for a constant image, as upstream).  scratch: evk_dense_rank_scratch_bytes(npix) bytes, 256-byte aligned. */
int64_t evk_dense_rank_scratch_bytes(int64_t npix);
int evk_dense_rank_f64(const double *image, int64_t npix, double *out, void *scratch, int64_t scratch_bytes, void *stream);
/* EventImage.get_image (image.py:391-394): out = (image - min) / (max - min), NaN-propagating like np.min / np.max.
 * scratch: evk_minmax_scratch_bytes() bytes. */
int64_t evk_minmax_scratch_bytes(void);
int evk_minmax_normalise_f64(const double *image, int64_t npix, double *out, double *scratch, void *stream);

/* ---- element-wise helpers of the host layer (evk_elem.hip, round 6) ---------------------------------------------
 * evk_polarity_weights_f32: pos[i] = p[i] > 0 ? 1 : 0, neg[i] = p[i] <= 0 ? 1 : 0 -- the two weight columns of
 *   events_to_neg_pos_voxel_torch (voxel_grid.py:173-174); either output may be NULL.
 * evk_abs_max: the BIT PATTERN of max |p| over a float32 (elem_bytes 4) or float64 (8) column into 8 bytes of device memory
 *   (a NaN anywhere gives a NaN pattern, as torch's max()); 0 for n == 0.
 * evk_abs: out[i] = |in[i]| (get_iwe's use_polarity=False, objectives.py:184-185); float32 or float64. */
int evk_polarity_weights_f32(const float *p, int64_t n, float *pos, float *neg, void *stream);
int evk_abs_max(const void *p, int elem_bytes, int64_t n, void *out8, void *stream);
/* the average-timestamp images around their events (image.py:266-283): evk_timestamp_planes_init_f32 sets the (4, plane_elems)
 * planes [time+, count+, time-, count-] to 0 / 1 / 0 / 1 (the counts START AT ONE upstream); evk_timestamp_finalise_f32 forms
 * pos = time+ / (count+ == 0 ? 1 : count+) and neg likewise (image.py:278-282), float32 divisions */
/* out[j] = np.searchsorted(a, keys[j]) (side 'left') for a sorted float32 (elem_bytes 4) / float64 (8) device column of n values
 * and m float64 device keys, compared in float64 as numpy does: the window bounds of events_to_voxel_timesync_torch /
 * voxel_grids_fixed_t_torch (voxel_grid.py:104-105) without copying the time column to the host */
int evk_searchsorted_left(const void *a, int elem_bytes, int64_t n, const double *keys, int64_t m, int64_t *out, void *stream);
int evk_timestamp_planes_init_f32(float *out4, int64_t plane_elems, void *stream);
int evk_timestamp_finalise_f32(const float *planes4, int64_t plane_elems, float *pos, float *neg, void *stream);
int evk_abs(const void *in, int elem_bytes, int64_t n, void *out, void *stream);
/* evk_narrow_f64_f32: out[i] = (float)(in[i] - offset), the subtraction in float64; *inexact (optional, caller-zeroed) |= 1
 * when some value is not exactly representable in float32 (also a NaN).  How the host layer takes the reference's float64
 * host arrays (xs, ys, ts, ps of objectives.py / events_cmax.py) onto the float32 path: columns whose values are float32-exact
 * as they are, the time stamps as differences from ts[-1] (DeviceEvents.from_arrays). */
int evk_narrow_f64_f32(const double *in, int64_t n, double offset, float *out, uint32_t *inexact, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Event filters (evk_select.hip): lib/util/event_util.py's clip_events_to_bounds (:61-94), get_events_from_mask (:96-109)
 * and remove_hot_pixels (:166-187) as one ORDER-PRESERVING stream compaction under a per-event predicate
 * ---------------------------------------------------------------------------------------------------------- */

/* coordinate kinds of the predicate columns x, y (and of evk_select_to_i32 / evk_mask_multiply_f64); image kinds of
 * evk_hot_pixels (EVK_SELECT_I32 / EVK_SELECT_F64) */
#define EVK_SELECT_I16 0
#define EVK_SELECT_I32 1
#define EVK_SELECT_I64 2
#define EVK_SELECT_F32 3
#define EVK_SELECT_F64 4
/* predicates: an event is KEPT when
 *   EVK_SELECT_BOX      minx <= x < maxx && miny <= y < maxy, compared in double (host_params = {minx, maxx, miny, maxy});
 *   EVK_SELECT_NOT_HOT  x, y are not an integral pixel of [0,w) x [0,h) whose byte in `image` (uint8 (h, w) hot map of
 *                       evk_hot_pixels) is non-zero;
 *   EVK_SELECT_MASK     image[yi, xi] >= host_params[0] for the float64 (h, w) mask `image`, xi / yi = x / y truncated toward
 *                       zero (astype(int)), a negative index wrapped once (numpy); an index still outside the mask, a NaN or
 *                       an infinity is counted in *oob (the reference raises IndexError) and the event is dropped. */
#define EVK_SELECT_BOX 0
#define EVK_SELECT_NOT_HOT 1
#define EVK_SELECT_MASK 2
/*   EVK_SELECT_RANDOM   event j is one of the uniform k-subset whose threshold evk_random_subset left in `image` (its state,
 *                       evk_hot_pixels_scratch_bytes() bytes): x, y and coord_kind are not read (x, y may be NULL), n < 2^32.
 *                       The outputs need hold only k elements: no position >= k is written. */
#define EVK_SELECT_RANDOM 3
/*   EVK_SELECT_FLAGS    byte j of `image` (n uint8 flags, e.g. the keep flags of evk_denoise_support / evk_denoise_refractory)
 *                       is non-zero: x, y and coord_kind are not read (x, y may be NULL). */
#define EVK_SELECT_FLAGS 4

/* scratch of evk_select_compact for n events (any content, 256-byte aligned) */
int64_t evk_select_scratch_bytes(int64_t n);
/* Column k < ncols of the payload (host arrays host_src / host_dst / host_elem_bytes: device pointers and element sizes 1, 2, 4
 * or 8) is copied byte for byte: host_dst[k][0 .. K) = the kept elements of host_src[k] in stream order.  index_out (may be
 * NULL) receives the kept int64 event indices.  Outputs hold up to n elements.  result: 3 device int64, written
 * [K, bits of column t_col's first kept element, bits of its last] (zero-extended; the last two only when K > 0 and t_col >= 0),
 * so that the caller reads the size and ts[0] / ts[-1] of the result in ONE transfer.  Three launches (count per 4096-event
 * chunk, scan, write): no inter-workgroup hand-over.  Columns are read element by element: any element-aligned start. */
int evk_select_compact(int pred, int coord_kind, const void *x, const void *y, int64_t n, const double *host_params,
                       const void *image, int h, int w, int ncols, const void *const *host_src, void *const *host_dst,
                       const int *host_elem_bytes, int t_col, int64_t *index_out, int64_t *result, void *scratch,
                       int64_t scratch_bytes, uint32_t *oob, void *stream);
/* x -> int32 pixel coordinates for the event image of remove_hot_pixels: *bad (caller-zeroed, may be NULL) |= 1 when a value
 * is not an integer (also NaN); an integer outside int32 becomes -1 (off every canvas: the image kernels count it in *oob). */
int evk_select_to_i32(int coord_kind, const void *in, int64_t n, int32_t *out, uint32_t *bad, void *stream);
/* remove_hot_pixels (event_util.py:177-183): hot[y * w + x] = 1 for the pixels the reference's loop "argmax, set to 0" picks in
 * num_hot rounds on the (h, w) top-left corner of `image` (int32 or float64, row pitch `pitch` elements), else 0.  Closed form:
 * pixels ordered by value descending (NaN above +inf, ties to the lower flat index), P = pixels > 0 or NaN; the first
 * min(num_hot, P) are hot; if num_hot > P one more: the lowest flat index among the pixels that are 0 after those picks, or,
 * when there is none, the argmax of the image.  num_hot <= 0 selects nothing.  A radix select on 96-bit keys (order-mapped
 * value, complemented index): 8 passes of 12-bit digits, 18 launches, all on the device.  h * w < 2^32 - 1.
 * scratch: evk_hot_pixels_scratch_bytes(), any content. */
int64_t evk_hot_pixels_scratch_bytes(void);
int evk_hot_pixels(const void *image, int image_kind, int h, int w, int pitch, int64_t num_hot, uint8_t *hot, void *scratch,
                   int64_t scratch_bytes, void *stream);
/* A uniform k-subset of the n candidates 0 .. n-1 (0 <= k <= n < 2^32): candidate i has the 96-bit key (64 bits of Philox word 0-1
 * of (seed, purpose, i), i); the k smallest keys are the subset.  The radix select of evk_hot_pixels finds the threshold and
 * leaves it, with seed and purpose, in `state` (evk_hot_pixels_scratch_bytes(), any content); evk_select_compact with
 * EVK_SELECT_RANDOM and image = state then keeps the subset in stream order, with no read-back in between. */
int evk_random_subset(uint64_t seed, uint32_t purpose, int64_t n, int64_t k, void *state, int64_t state_bytes, void *stream);
/* clip_events_to_bounds(set_zero=True) (event_util.py:80-84): out[i] = (double)in[i] * mask[i] (mask of evk_bounds_mask_f64);
 * offset != 0 is added to (double)in[i] first (a time column stored relative to it) */
int evk_mask_multiply_f64(int kind, const void *in, int64_t n, double offset, const double *mask, double *out, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Event denoising (evk_denoise.hip): the neighbour-support count of the background-activity filter (Delbruck; with a support
 * threshold above 1, Guo & Delbruck's spatio-temporal correlation filter) and the refractory-period filter.
 *
 * Events i = 0 .. n-1 are in stream order, each with an integer pixel (x_i, y_i) in [0, w) x [0, h), a time t_i and -- when
 * classes == 2 -- a polarity class c_i (cls[i] != 0; the host layer passes p_i > 0).  Time differences are formed in double
 * from the stored values (integer columns convert to double first).  Time stamps need not be sorted: "earlier" always means
 * a smaller stream index.
 *   support_i   = the number of pixels q of the (2r+1)^2 window around (x_i, y_i), clipped to the sensor, without the centre
 *                 unless include_self, for which last(q, i) -- the event with the largest index j < i at pixel q, and of class
 *                 c_i when classes == 2 -- exists and t_i - t_last <= dt.  A negative difference counts as within dt (what a
 *                 timestamp map does on unsorted input); dt = 0 keeps exact ties.  Pixels, not events: at most (2r+1)^2.
 *   background-activity filter: keep event i iff support_i >= min_support.
 *   refractory filter: per pixel (per pixel and class when classes == 2) the first event is kept; a later event i is kept iff
 *                 t_i - t_k >= refractory, k the last KEPT earlier event of that pixel (and class).
 * Pass structure: evk_denoise_group writes a 32-bit key class * h*w + y*w + x and the index of every event, sorts the pairs
 * stably by key (hipcub::DeviceRadixSort::SortPairs over the key's significant bits) into order[] -- the indices grouped by
 * key, ascending inside a key -- and builds the run table start[K + 1], K = classes * h * w, empty keys allowed.  The support
 * pass runs one thread per event and binary-searches each window pixel's run for the predecessor of i; the
 * refractory pass walks each run, one thread per run shorter than EVK_DENOISE_WAVE_RUN events and a whole wave per longer run
 * (64 consecutive times per load, the chain resolved in registers).  The flags then go through evk_select_compact
 * (EVK_SELECT_FLAGS).  The caller owns all memory; every call is ordered on `stream`.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_DENOISE_MAX_RADIUS 3
#define EVK_DENOISE_WAVE_RUN 4096
/* the order in which the threads of the support pass take the events: stream order (coalesced key and time loads) or pixel order
 * (thread p takes event order[p]: the threads of a wave search the runs of the same few pixels); the default is pixel order */
#define EVK_DENOISE_WALK_DEFAULT 0
#define EVK_DENOISE_WALK_STREAM 1
#define EVK_DENOISE_WALK_PIXEL 2
/* scratch of one grouping (256-byte aligned, any content): n < 2^31 events, classes 1 or 2, classes * h * w < 2^31 - 1;
 * negative (EVK_EINVAL) otherwise */
int64_t evk_denoise_scratch_bytes(int64_t n, int h, int w, int classes);
/* x, y: int32 pixel columns (evk_select_to_i32); cls: n uint8 class flags (read when classes == 2, else may be NULL).  A pixel
 * outside [0, w) x [0, h) is counted in *oob and grouped under key 0 (the host layer raises ValueError). */
int evk_denoise_group(const int32_t *x, const int32_t *y, const uint8_t *cls, int64_t n, int h, int w, int classes, void *scratch,
                      int64_t scratch_bytes, uint32_t *oob, void *stream);
/* t: the time column, t_kind one of EVK_SELECT_I16 .. EVK_SELECT_F64; n, h, w, classes and scratch those of the grouping.
 * support[i] = support_i (n uint8); keep (may be NULL): keep[i] = support_i >= min_support.  dt >= 0 (not NaN), radius
 * 1 .. EVK_DENOISE_MAX_RADIUS, min_support 0 .. (2 radius + 1)^2, walk one of EVK_DENOISE_WALK_*. */
int evk_denoise_support(int t_kind, const void *t, int64_t n, int h, int w, int classes, double dt, int radius, int include_self,
                        int min_support, int walk, void *scratch, uint8_t *support, uint8_t *keep, void *stream);
/* keep[i] = 1 / 0 by the refractory filter (n uint8; every byte is written when no pixel was out of range).  refractory >= 0
 * (not NaN).  wave_run: the run length from which a whole wave walks a run, <= 0 for EVK_DENOISE_WAVE_RUN. */
int evk_denoise_refractory(int t_kind, const void *t, int64_t n, int h, int w, int classes, double refractory, int wave_run,
                           void *scratch, uint8_t *keep, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Time surfaces (evk_tsurf.hip): the exponentially decayed surface of active events (SAE) at a query, the per-event local time
 * surface of HOTS (Lagorce et al., PAMI 2017) and the cell-averaged histograms of HATS (Sironi et al., CVPR 2018).
 *
 * Events, pixels, times and polarity classes (p > 0) are those of "Event denoising"; "earlier" means a smaller stream index, and
 * ages are formed in double from the stored time values (a common time offset cancels).
 *   last(q, c, m) = the event with the largest index j < m at pixel q (of class c when the grouping has two classes).
 *   An age is +inf when there is no such event or q lies off the sensor.  Ages are not clamped: on unsorted input an age can
 *   be negative, which is what a timestamp-map loop gives.
 *   The value of an age a: EVK_TSURF_EXP (float)exp(-a / tau), EVK_TSURF_LINEAR (float)max(0, 1 - a / tau), both evaluated
 *   in double; EVK_TSURF_AGE a itself as a double.  +inf gives 0, 0 and +inf.  tau > 0.
 *   global   S[k, c, y, x] = value(T_k - t[last((x, y), c, m_k)]) for query k with the cut m_k in 0 .. n and the reference time
 *            T_k = t_refs[k], or t[m_k - 1] when t_refs is NULL.  m_k = 0 gives an empty surface.  Shape (nq, classes, h, w).
 *   local    L[i, c, dy, dx] from the age t_i - t[last((x_i + dx, y_i + dy), c, i)], |dx|, |dy| <= radius.  split = 0: one channel,
 *            the event's own key (every event of the pixel with classes == 1, the class of event i with classes == 2); split = 1
 *            (classes == 2): channel 0 is p <= 0, channel 1 is p > 0.  include_self puts age 0 at the centre of the event's own
 *            class.  With `select` (m int64 indices in [0, n), any order, repeats allowed) row r of the output is event
 *            select[r], otherwise row i is event i.  Shape (rows, channels, 2r+1, 2r+1).
 *   HATS     for event i of class q in the cell g (cell x cell pixels, smaller at the right and bottom edge):
 *            T_i(z) = the sum of exp(-(t_i - t_j) / tau) over the events j < i of class q at pixel_i + z, that pixel inside the
 *            sensor AND inside cell g (the paper's per-cell memory), with t_i - t_j <= dt;  h[g, q, z] = the sum of T_i(z) over
 *            the events of (g, q), divided by their number with `normalise` (an empty cell gives zeros).  The time column must be
 *            non-decreasing (evk_tsurf_check_sorted), sums are formed in double.  Shape (cells_y, cells_x, 2, 2r+1, 2r+1) float32,
 *            counts (may be NULL) (cells_y, cells_x, 2) int32.
 * Pass structure: all three run on the grouping of evk_denoise_group (same n, h, w, classes and scratch).  The global pass runs one
 * thread per output element: the lower bound of m_k in the pixel's run and one gathered time.  The local pass runs one lane per
 * output element with the events in pixel order, so that a wave searches the runs of a few pixels and stores whole patches.  The
 * HATS pass first gathers the times into run order (t_scratch), then runs one wave per (cell, class) with the lanes on the window
 * elements: the wave walks the cell's pixels in row-major order and every run in ascending order, each lane with two forward-only
 * positions in its neighbour's run.  Nothing is accumulated with atomics: results repeat bit for bit.  One crowded pixel makes
 * one wave of the HATS pass slow; the cells are not balanced.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_TSURF_MAX_RADIUS 4
#define EVK_TSURF_EXP 0
#define EVK_TSURF_LINEAR 1
#define EVK_TSURF_AGE 2
/* t_scratch of evk_tsurf_hats for n events (256-byte aligned, any content); negative (EVK_EINVAL) for n outside 0 .. 2^31 - 1 */
int64_t evk_tsurf_scratch_bytes(int64_t n);
/* *unsorted (device, caller-zeroed) += the number of i with t[i + 1] < t[i]; t_kind one of EVK_SELECT_I16 .. EVK_SELECT_F64 */
int evk_tsurf_check_sorted(int t_kind, const void *t, int64_t n, uint32_t *unsorted, void *stream);
/* cuts: nq device int64 (a value outside 0 .. n is clamped); t_refs: nq device doubles in the time base of t, or NULL;
 * out: nq * classes * h * w float32 (float64 with EVK_TSURF_AGE) */
int evk_tsurf_global(int t_kind, const void *t, int64_t n, int h, int w, int classes, int64_t nq, const int64_t *cuts,
                     const double *t_refs, int decay, double tau, void *scratch, void *out, void *stream);
/* select: m device int64 or NULL (then every event, m is not read); an index outside [0, n) gives a row of empty ages (the host
 * layer raises IndexError first).  out: rows * (split ? 2 : 1) * (2 radius + 1)^2 float32 (float64 with EVK_TSURF_AGE) */
int evk_tsurf_local(int t_kind, const void *t, int64_t n, int h, int w, int classes, int radius, int decay, double tau, int split,
                    int include_self, const int64_t *select, int64_t m, void *scratch, void *out, void *stream);
/* scratch: a grouping with classes == 2; t_scratch: evk_tsurf_scratch_bytes(n) bytes; cell >= 1; dt >= 0 (not NaN) */
int evk_tsurf_hats(int t_kind, const void *t, int64_t n, int h, int w, int cell, int radius, double tau, double dt, int normalise,
                   void *scratch, void *t_scratch, int64_t t_scratch_bytes, float *out, int32_t *counts, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Corner detection (evk_corner.hip): the eFAST arc test (Mueggler, Bartolozzi, Scaramuzza, BMVC 2017) and the Harris score of a
 * binary patch (Vasco, Glover, Bartolozzi, IROS 2016), event by event.
 *
 * Events, pixels, times and polarity classes (p > 0) are those of "Event denoising"; "earlier" means a smaller stream index, the
 * times may be unsorted and are compared as doubles after an exact conversion of the column.  classes == 2: an event only sees its
 * own class; classes == 1: every event of the pixel.
 *   last(q, i)  = the last event of the class of event i at pixel q with an index below i, or none.
 *   border      an event with x < EVK_CORNER_BORDER, x >= w - EVK_CORNER_BORDER, y < EVK_CORNER_BORDER or y >= h - EVK_CORNER_BORDER
 *               is never a corner and its Harris score is NaN: on a sensor with h < 9 or w < 9 nothing is a corner.
 *   selection   with `select` (rows int64 indices in [0, n), any order, repeats allowed) element r of the output is event
 *               select[r], otherwise element i is event i.  Every event forms the history.
 *   eFAST       v(q) = the time of last(q, i), -inf when there is none, on two circles around the event, as (dx, dy) in this
 *               cyclic order:
 *                 C3 (16): (0,3)(1,3)(2,2)(3,1)(3,0)(3,-1)(2,-2)(1,-3)(0,-3)(-1,-3)(-2,-2)(-3,-1)(-3,0)(-3,1)(-2,2)(-1,3)
 *                 C4 (20): (0,4)(1,4)(2,3)(3,2)(4,1)(4,0)(4,-1)(3,-2)(2,-3)(1,-4)(0,-4)(-1,-4)(-2,-3)(-3,-2)(-4,-1)(-4,0)(-4,1)
 *                          (-3,2)(-2,3)(-1,4)
 *               A circle of m values has an arc of length L if there is a start s such that the minimum of v[(s + j) mod m],
 *               j < L, is STRICTLY greater than the maximum of the other m - L values.  Event i is a corner iff it is off the
 *               border, C3 has an arc of some length 3 .. 6 and C4 has an arc of some length 4 .. 8.  So an arc never contains a
 *               pixel that has not fired, and a tie between an arc element and an outside element defeats the arc: the published
 *               detector's rules for positive time stamps on a zero-initialised surface.  Only comparisons: exact.
 *   Harris      the binary patch b[dy + 4][dx + 4], |dx|, |dy| <= 4: the centre is 1; elsewhere 1 iff j = last((x + dx, y + dy), i)
 *               exists and is recent: EVK_CORNER_WINDOW_COUNT j >= i - n_last (among the last n_last events of the stream),
 *               EVK_CORNER_WINDOW_TIME t_i - t_j <= dt in double.  (Vasco et al. keep one queue per polarity: with balanced
 *               polarities n_last here corresponds to about n_last / 2 there.)  With S = [1, 4, 6, 4, 1], D = [-1, -2, 0, 2, 1], for
 *               a, c in 0 .. 4:  Ix[a][c] = sum_{u,v} S[u] D[v] b[a + u][c + v],  Iy[a][c] = sum_{u,v} D[u] S[v] b[a + u][c + v]
 *               (integers, at most 48 in magnitude); the window g[a][c] = exp(-((a - 2)^2 + (c - 2)^2) / 2), normalised to sum 1 in
 *               double;  A = sum g Ix^2 / 144, B = sum g Iy^2 / 144, C = sum g Ix Iy / 144 (the gradients scaled by the largest
 *               Sobel coefficient, 12);  score = A B - C^2 - k (A + B)^2, evaluated in double -- the sums over (a, c) in
 *               row-major order, then (A B - C C) - k ((A + B)(A + B)) -- and stored as float32.
 * Pass structure: both run on the grouping of evk_denoise_group (same n, h, w, classes and scratch).  A workgroup takes 64 events
 * per step, in pixel order or in the order of `select`; each event is decoded once, its look-ups (36 and 80 predecessor
 * searches) are spread over the four waves with lane = event, the circle times or patch bits stay in LDS, and only the flag
 * or the score is stored.  No atomics: results repeat bit for bit.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_CORNER_BORDER 4
#define EVK_CORNER_WINDOW_COUNT 0
#define EVK_CORNER_WINDOW_TIME 1
/* select: rows device int64 or NULL (then every event, rows is not read beyond rows >= 0); an index outside [0, n) gives 0 (the
 * host layer raises IndexError first).  out: one uint8 (1 corner, 0 not) per output element */
int evk_corner_fast(int t_kind, const void *t, int64_t n, int h, int w, int classes, const int64_t *select, int64_t rows,
                    const void *scratch, uint8_t *out, void *stream);
/* window one of EVK_CORNER_WINDOW_*; n_last >= 1 and dt >= 0 (not NaN) whichever window is used; k not NaN.  out: one float32 per
 * output element, NaN on the border and for an index outside [0, n) */
int evk_corner_harris(int t_kind, const void *t, int64_t n, int h, int w, int classes, int window, int64_t n_last, double dt,
                      double k, const int64_t *select, int64_t rows, const void *scratch, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Plane-fit flow (evk_planeflow.hip): the local plane fit on the surface of active events (Benosman et al., "Event-based visual
 * flow", TNNLS 2014; "LocalPlanes" in Rueckauer & Delbruck 2016) with the event lifetime of Mueggler et al. (ICRA 2015), event by
 * event, and the per-pixel average of the per-event flow as a dense field.
 *
 * Events, pixels, polarity classes (p > 0), "earlier" (a smaller stream index) and last(q, i) are those of "Corner detection";
 * the times may be unsorted and are converted exactly to double.
 *   parameters  radius r in 1 .. EVK_PLANEFLOW_MAX_RADIUS; dt >= 0; min_samples m in 3 .. (2r + 1)^2; threshold th > 0 or absent
 *               (use_threshold = 0); iterations R in 0 .. EVK_PLANEFLOW_MAX_ITERATIONS; max_speed > 0 or absent (use_max_speed = 0).
 *   samples     for (dy, dx) row-major (dy outer, both from -r to r) and q = (x_i + dx, y_i + dy): sample k is in use iff q is on
 *               the sensor, j = last(q, i) exists and t_i - t_j <= dt in double; its value is tau_k = t_j - t_i.  The centre (0, 0)
 *               is always in use with tau = 0: it stands for the event itself, not for its predecessor.  The window is clipped
 *               to the sensor; there is no border rule.
 *   fit         over the samples in use: the integer sums n, sx, sy, sxx, sxy, syy of 1, dx, dy, dx^2, dx dy, dy^2 (exact in
 *               any order) and the double sums st = sum tau_k, sxt = sum dx_k tau_k, syt = sum dy_k tau_k, each accumulated in
 *               row-major order of k from 0.0 without fused multiply-add.  Cofactors
 *                 c11 = syy n - sy sy      c12 = sx sy - sxy n      c13 = sxy sy - syy sx
 *                 c22 = sxx n - sx sx      c23 = sxy sx - sxx sy    c33 = sxx syy - sxy sxy
 *               and the determinant D = sxx c11 + sxy c12 + sx c13 (an integer below 2^53: exact).  The fit FAILS iff n < m or
 *               D == 0 (collinear samples).  Otherwise, in double,
 *                 a = ((c11 sxt + c12 syt) + c13 st) / D
 *                 b = ((c12 sxt + c22 syt) + c23 st) / D
 *                 c = ((c13 sxt + c23 syt) + c33 st) / D
 *               the plane tau ~ a dx + b dy + c.
 *   rejection   only with th, at most R rounds: the residual e_k = |((a dx_k + b dy_k) + c) - tau_k|; every non-centre sample in
 *               use with e_k > th is dropped; if nothing was dropped, stop, otherwise refit on the rest.  A failed refit makes the
 *               event invalid.
 *   result      g = a a + b b.  Valid iff the last fit succeeded, g > 0 and, with max_speed, 1.0 / g <= max_speed * max_speed.
 *               vx = (float)(a / g), vy = (float)(b / g): the normal flow in pixels per unit of t.  lifetime = (float)sqrt(g): time
 *               per pixel.  An invalid event has NaN in all three and valid = 0.
 *   selection   as in "Corner detection": with `select` row r of the output is event select[r], otherwise row i is event i.
 *   field       for every pixel the events there whose flow is valid -- with two classes those of class p <= 0 first, then p > 0,
 *               each in ascending stream index; with one class in ascending index --: the stored float32 vx, vy are widened to
 *               double and summed in that order; field[:, y, x] = (float)(sum / count), 0 where count == 0.
 * Pass structure: both run on the grouping of evk_denoise_group (same n, h, w, classes and scratch).  The fit takes 64 events per
 * workgroup and step, in pixel order or in the order of `select`; the (2r + 1)^2 - 1 predecessor searches of an event are spread
 * over the four waves with lane = event, tau and the in-use flags stay in LDS, three waves form one double sum each in the defined
 * order while the fourth forms the integer sums, and the residual test is spread like the look-ups.  The field pass takes one
 * lane per pixel and walks the pixel's run(s): one crowded pixel makes one lane slow; the pixels are not balanced.  No atomics:
 * results repeat bit for bit.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_PLANEFLOW_MAX_RADIUS 4
#define EVK_PLANEFLOW_MAX_ITERATIONS 8
/* select: rows device int64 or NULL (then every event, rows is not read beyond rows >= 0); an index outside [0, n) gives an
 * invalid row (the host layer raises IndexError first).  flow: rows x 2 float32 (vx, vy); lifetime: rows float32, may be NULL;
 * valid: rows uint8.  threshold and max_speed must not be NaN even when they are not used; iterations is not used without a
 * threshold. */
int evk_planeflow_fit(int t_kind, const void *t, int64_t n, int h, int w, int classes, int radius, double dt, int min_samples,
                      int use_threshold, double threshold, int iterations, int use_max_speed, double max_speed,
                      const int64_t *select, int64_t rows, const void *scratch, float *flow, float *lifetime, uint8_t *valid,
                      void *stream);
/* flow (n x 2 float32) and valid (n uint8): what evk_planeflow_fit gave without `select` on the same grouping.  field: 2 x h x w
 * float32 (vx plane, vy plane); count: h x w int32.  With n == 0 the scratch is not read and the field is zero. */
int evk_planeflow_field(int64_t n, int h, int w, int classes, const void *scratch, const float *flow, const uint8_t *valid,
                        float *field, int32_t *count, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Intensity reconstruction (evk_reconstruct.hip): the leaky event integrator (the high-pass filter) and the complementary filter
 * of Scheerlinck, Barnes & Mahony, "Continuous-time Intensity Estimation Using Event Cameras" (ACCV 2018): a per-pixel estimate
 * of the log intensity from the events alone, or from the events and the latest frame.
 *
 * Events, pixels and times are those of "Event denoising" on a grouping with one class.  The definition holds per pixel; all
 * arithmetic is in double, and time differences are formed in double from the stored column (integer columns convert first).
 *   inputs      alpha >= 0 (finite), in 1 / unit of t; contrasts c_on > 0 and c_off > 0; events with non-decreasing t
 *               (evk_tsurf_check_sorted); optionally nf >= 1 frames (nf, h, w), already in the log domain, with strictly increasing
 *               times frame_ts[nf]; a start time t_start and a start state initial (h, w), NULL for zeros.
 *   target      F(t) = 0 without frames; with frames F(t) = frames[f] for frame_ts[f] <= t < frame_ts[f + 1], frames[0] also for
 *               every t < frame_ts[1] and frames[nf - 1] from frame_ts[nf - 1] on.
 *   evolution   L(t_start) = initial.  Between events dL/dt = -alpha (L - F(t)): advancing from a to b under a constant target F
 *               gives L(b) = F + (L(a) - F) exp(-alpha (b - a)), and an advance is split at every frame time inside (a, b).  With
 *               alpha == 0 an advance leaves L as it is: direct integration, the frames have no influence.  At event j with
 *               t_j >= t_start: L += c_on if the event is positive, else L -= c_off.  Events with t_j < t_start do not count
 *               (the caller passes their number as start_cut).
 *   queries     nq >= 1 non-decreasing times T_k >= t_start with cuts m_k in 0 .. n: out[k, y, x] = L(T_k) after exactly the
 *               events with an index below m_k, rounded once to float32.  The host layer passes m_k = the number of events with
 *               t < T_k (evk_searchsorted_left, as the time surfaces do): an event or a frame at exactly a query time needs no tie
 *               rule.  With cuts given as indices it passes T_k = t[m_k - 1].
 * The system is linear, so L(T) = P(T) + E(T): P the event-free solution from `initial` under F, E(T) = sum_j c_j exp(-alpha (T -
 * t_j)) over the counted events, c_j = c_on or -c_off.  The kernel evaluates this split: the terms of a run are independent, the
 * sum of a run is formed in a fixed order, and from one query to the next E_k = exp(-alpha (T_k - T_{k-1})) E_{k-1} + (the terms
 * of the new events).  Against the literal recurrence the result differs by float64 reassociation only: at most about
 * (events of the pixel + nq + nf) 2^-53 A with A = |initial| + max_f |frames[f]| + sum_j |c_j| exp(-alpha (T_k - t_j)).
 * Pass structure: one kernel on the grouping of evk_denoise_group (classes == 1; same n, h, w and scratch).  A wave takes 64
 * consecutive pixels; a lane walks the run of its pixel when it is shorter than wave_run events, four events loaded ahead of their
 * exps, and finds each query's cut as the run's ascending indices reach m_k; the longer runs are then taken by the whole wave,
 * 256 consecutive events per step, the cut found as a lower bound, the 64 lanes' sums joined once per query by a wave reduction
 * in a fixed order.  The lane that owns the pixel (lane 0 on the wave path) forms P inline and stores (float)(P + E): neighbouring
 * lanes store neighbouring pixels.  No atomics: results repeat bit for bit.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_RECONSTRUCT_WAVE_RUN 1024
/* t, n, h, w and scratch: those of the grouping (classes == 1); with n == 0 the scratch is not read (but must be given).
 * pos_flags: n uint8, != 0 for a positive event.  initial: h * w doubles or NULL; frames: nf * h * w doubles and frame_ts: nf
 * doubles, both NULL when nf == 0; cuts: nq int64 (a value outside 0 .. n is clamped); t_refs: nq doubles in the time base of t;
 * start_cut in 0 .. n: the number of events with t < t_start.  All arrays are device memory.  wave_run: the run length from which
 * a whole wave takes a run, <= 0 for EVK_RECONSTRUCT_WAVE_RUN.  out: nq * h * w float32.  EVK_EINVAL, before any device work, for a
 * missing pointer, nq < 1, alpha negative, NaN or infinite, a contrast that is not positive and finite, a NaN t_start, nf < 0,
 * start_cut outside 0 .. n or a scratch that is not 256-byte aligned. */
int evk_reconstruct(int t_kind, const void *t, const uint8_t *pos_flags, int64_t n, int h, int w, double alpha, double c_on,
                    double c_off, double t_start, const double *initial, int nf, const double *frames, const double *frame_ts,
                    int64_t nq, const int64_t *cuts, const double *t_refs, int64_t start_cut, int wave_run, const void *scratch,
                    float *out, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Event simulation (evk_simulate.hip): events from log-intensity frames by the threshold-crossing model (ESIM, Rebecq et al.
 * 2018; the noise-free core of v2e) -- the forward model of which evk_reconstruct with alpha == 0 is the inverse.
 *
 *   inputs      frames (nf, h, w), already in the log domain, nf >= 2; frame_ts[nf] strictly increasing finite times, none of
 *               them -0.0 (the host layer adds +0.0); contrasts c_on > 0 and c_off > 0, each a scalar or a per-pixel (h, w) map;
 *               refractory >= 0; a start state: reference (h, w), NULL for frames[0], and last_event_ts (h, w), NULL for -inf.
 *   arithmetic  IEEE double, every operation below one rounding (no contraction into fused multiply-adds, no fast-math).  The log
 *               intensity of a pixel is linear between consecutive frames.
 *   walk        Per pixel: R = reference, tl = last_event_ts.  For each interval f = 0 .. nf - 2 in order, with L0 = frames[f],
 *               L1 = frames[f + 1], T0 = frame_ts[f], T1 = frame_ts[f + 1], d = L1 - L0, dT = T1 - T0: if d is not finite or is
 *               zero the interval emits nothing and leaves R as it is.  Otherwise, while fewer than EVK_SIMULATE_MAX_STEPS
 *               crossings have been taken in this interval:
 *                 if d > 0 and R + c_on <= L1:       R = R + c_on,  p = +1
 *                 else if d < 0 and R - c_off >= L1: R = R - c_off, p = -1
 *                 else stop;
 *                 frac = (R - L0) / d, clamped to [0, 1] (below 0 -> 0, above 1 -> 1); t = T0 + frac * dT;
 *                 the event (x, y, t, p) is emitted iff t - tl >= refractory; then tl = t.
 *               A crossing inside the refractory period moves R and tl but emits nothing.  If the step limit ends the loop while
 *               a further crossing is still due, the pixel-interval counts as an overflow.  The limit is part of the definition:
 *               it is what keeps a pixel from spinning on a huge jump, a tiny contrast or a contrast below the ulp of R.
 *   order       ascending t; equal t in the order of the pixel index y * w + x; equal t at one pixel in emission order.  Every t
 *               lies in [frame_ts[0], t_max] with t_max = the largest T0 + (T1 - T0) as rounded, which is frame_ts[nf - 1]
 *               wherever those sums are exact (always for positive times with T1 <= 2 T0).
 *   state out   R and tl of every pixel after the last interval.  A next chunk that starts with this chunk's last frame, reference
 *               = R and last_event_ts = tl continues the walk exactly.
 * Pass structure: evk_simulate_count (one lane per pixel walks the intervals: the pixel's event count), an exclusive scan of the
 * counts over the pixel index by the caller, who reads the total and the report back -- the one synchronisation, needed to size
 * the output --, evk_simulate_emit (the identical walk: the events of pixel q from offsets[q] on in emission order, and the
 * state), evk_simulate_sort (a stable radix sort of the pixel-major pairs by time, which makes stability the tie rule, and one
 * gather into the columns).  The sort key of t is its order-preserving 64-bit image minus that of frame_ts[0], sorted from bit
 * 0 over the bits in which [frame_ts[0], t_max] can differ (at least 8): the range needs no device reduction and the gather gets
 * t back from the key exactly.  No atomics on the output path: results repeat bit for bit.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_SIMULATE_MAX_STEPS 65536
/* All arrays are device memory of doubles unless stated.  c_on_map / c_off_map: h * w contrasts or NULL for the scalar (which is
 * then not read when the map is given).  counts: h * w uint32 (saturating).  report: 2 uint64, zeroed by the call: [0] the
 * overflowed pixel-intervals, [1] the pixels with a map contrast that is not positive and finite (such a pixel is not walked).
 * EVK_EINVAL, before any device work, for a missing pointer, nf < 2, h <= 0 or w <= 0, more than 2^32 - 1 pixels, a scalar
 * contrast in use that is not positive and finite, or a negative or NaN refractory. */
int evk_simulate_count(const double *frames, const double *frame_ts, int nf, int h, int w, double c_on, double c_off,
                       const double *c_on_map, const double *c_off_map, double refractory, const double *reference,
                       const double *last_event_ts, uint32_t *counts, uint64_t *report, void *stream);
/* offsets: h * w int64, the exclusive scan of counts; total: their sum, 0 .. 2^31 - 1 (no store goes outside [0, total) whatever
 * offsets holds).  t_first = frame_ts[0].  keys: total uint64; vals: total uint32 holding pixel * 2 + (p > 0), or uint64 when
 * wide != 0 or h * w > 2^31.  reference_out, last_event_ts_out: h * w doubles, always written.  EVK_EINVAL as above, and for a
 * total outside that range or a NaN t_first. */
int evk_simulate_emit(const double *frames, const double *frame_ts, int nf, int h, int w, double c_on, double c_off,
                      const double *c_on_map, const double *c_off_map, double refractory, const double *reference,
                      const double *last_event_ts, const int64_t *offsets, int64_t total, double t_first, int wide, uint64_t *keys,
                      void *vals, double *reference_out, double *last_event_ts_out, void *stream);
/* keys, vals, total, wide, t_first: those of evk_simulate_emit; t_max >= every event time (see "order").  xs, ys, ps: total int64
 * (p = +1 / -1); ts: total doubles.  scratch: evk_simulate_sort_scratch_bytes(...) bytes, 256-byte aligned.  total == 0 does
 * nothing.  EVK_EINVAL for a missing pointer, a total outside 0 .. 2^31 - 1 (hipcub's item count is an int), h <= 0, w <= 0,
 * more than 2^32 - 1 pixels, or t_max < t_first or NaN. */
int64_t evk_simulate_sort_scratch_bytes(int64_t total, int h, int w, int wide, double t_first, double t_max);
int evk_simulate_sort(const uint64_t *keys, const void *vals, int64_t total, int h, int w, int wide, double t_first, double t_max,
                      void *scratch, int64_t scratch_bytes, int64_t *xs, int64_t *ys, double *ts, int64_t *ps, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Event-based multi-view stereo (evk_emvs.hip): depth from a moving camera with known poses (EMVS, Rebecq et al., IJCV 2018).
 * Every event is a ray through a disparity space image (DSI), a (nd, h, w) volume of depth planes in front of a reference view;
 * a cell counts the rays through it; depth is read off the maxima.
 *
 *   packets     packet j is events [j ps, min((j + 1) ps, n)) in stream order, ps = min(packet_size, max(n, 1)); its time is ts
 *               of event j ps + cnt_j / 2 (integer division).  The caller turns the times into the packet table on the host: 12
 *               doubles per packet, M = R_ref^T R_j K^-1 row-major (9) and C = R_ref^T (c_j - c_ref) (3).
 *   arithmetic  IEEE double, every operation one rounding in the order written (no fused multiply-adds, no fast-math).
 *   ray         per event (x, y) of packet j:  d_k = (M_k0 x + M_k1 y) + M_k2, k = 0, 1, 2; the event is skipped unless d_2 > 0;
 *               a = d_0 / d_2, b = d_1 / d_2.
 *   plane i     Z = depths[i], rZ = inv_depths[i] (the caller's table of 1.0 / Z): s = Z - C_2, the plane is skipped unless
 *               s > 0; u = (fx (C_0 + s a)) rZ + cx, v = (fy (C_1 + s b)) rZ + cy with the reference view's fx, fy, cx, cy.
 *   nearest     iu = floor(u + 0.5), iv = floor(v + 0.5): raw[i, iv, iu] += 1 when 0 <= iu < w and 0 <= iv < h.
 *   bilinear    x0 = floor(u), fu = u - x0, y0 = floor(v), fv = v - y0; the corners (x0, y0), (x0 + 1, y0), (x0, y0 + 1),
 *               (x0 + 1, y0 + 1) get q = rint(256 wgt), ties to even, of wgt = (1 - fu)(1 - fv), fu (1 - fv), (1 - fu) fv, fu fv,
 *               each corner on its own when it lies inside.
 *               A u or v that is NaN or infinite votes nowhere.
 *   cells       uint32; one raw unit is one vote (nearest) or 1 / 256 vote (bilinear).  Integer adds commute: the volume is the
 *               same bits whatever the order of the votes and however the work is cut.  n < 2^31; bilinear n < 2^24 (a cell
 *               cannot wrap).
 *   depth map   conf = max_i raw[i], peak = the smallest i that attains it, -1 where conf == 0.  S = the sum of conf over the
 *               (2 r + 1)^2 window, zero outside the image; area = (2 r + 1)^2 always; mask = conf area - S > threshold area in
 *               64-bit integers (threshold in raw units).  index = peak where mask, else -1; with median_size 3 or 5 the lower
 *               median (element (k - 1) / 2 of the k sorted values) of the peaks of the masked pixels of the window, the pixel
 *               itself included.  depth = depths[index], NaN where index is -1.
 * Kernel structure: one pass per event for (a, b); then a workgroup per (plane, tile, event chunk) that keeps its tile -- a band
 * of evk_emvs_band_rows rows, cut into evk_emvs_band_cols columns only when a row exceeds the LDS -- as uint32 cells in LDS and
 * flushes the non-zero cells with global integer adds.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_EMVS_NEAREST 0
#define EVK_EMVS_BILINEAR 1
#define EVK_EMVS_BILINEAR_MAX_EVENTS 16777216
/* ts: n device floats (EVK_T_F32) or doubles (EVK_T_F64); packet_ts: ceil(n / ps) device doubles.  n == 0 does nothing.
 * EVK_EINVAL, before any device work, for another t_kind, n < 0 or n >= 2^31, packet_size < 1 or a missing pointer. */
int evk_emvs_packet_times(int t_kind, const void *ts, int64_t n, int64_t packet_size, double *packet_ts, void *stream);
/* The tile of the vote kernel for an h x w plane, and the event chunks a call with chunks == 0 is cut into (EVK_EINVAL for sizes
 * evk_emvs_votes refuses). */
int evk_emvs_band_rows(int h, int w);
int evk_emvs_band_cols(int h, int w);
int evk_emvs_chunks(int64_t n, int nd, int h, int w);
/* xs, ys: n device floats or doubles (xy_kind: EVK_T_F32 / EVK_T_F64), any values; packets: n_packets x 12 device doubles,
 * n_packets == ceil(n / ps); depths, inv_depths: nd device doubles; mode: EVK_EMVS_NEAREST / EVK_EMVS_BILINEAR; chunks: the
 * event chunks, 0 for evk_emvs_chunks(...) (the result does not depend on it); rays: 2 n device doubles of scratch; raw:
 * nd x h x w uint32, zeroed by the call.  n == 0 only zeroes raw.  EVK_EINVAL, before any device work, for another kind or mode,
 * n < 0, n >= 2^31, bilinear n >= 2^24, packet_size < 1, a wrong n_packets, nd < 1, h < 1, w < 1, h w > 2^31 - 1,
 * nd h w > 2^40, fx or fy not positive and finite, cx or cy not finite, chunks outside 0 .. 65535 or a missing pointer. */
int evk_emvs_votes(int xy_kind, const void *xs, const void *ys, int64_t n, int64_t packet_size, const double *packets,
                   int64_t n_packets, const double *depths, const double *inv_depths, int nd, double fx, double fy, double cx,
                   double cy, int h, int w, int mode, int chunks, double *rays, void *raw, void *stream);
/* raw: nd x h x w uint32; threshold: raw units, 0 .. 2^45; radius 0 .. 16; median_size 0, 3 or 5.  Outputs, h x w each:
 * confidence uint32, peak int32, mask uint8 (0 / 1), index int32, depth doubles.  EVK_EINVAL, before any device work, for sizes
 * as above, a radius, threshold or median_size outside those, or a missing pointer. */
int evk_emvs_depth_map(const void *raw, const double *depths, int nd, int h, int w, int radius, int64_t threshold, int median_size,
                       void *confidence, void *peak, void *mask, void *index, double *depth, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Event stereo (evk_stereo.hip): disparity from two rectified, time-synchronised event cameras by block matching on quantised
 * time surfaces (the mapping step of ESVO, Zhou et al., T-RO 2021, and the time-surface stereo before it).  Rectified: a scene
 * point at (x, y) on the left lies at (x - d, y) on the right, d >= 0.  Both sensors are h x w.
 *
 *   ages        A[k, c, y, x], the double age of the last event of class c before query k: evk_tsurf_global with EVK_TSURF_AGE,
 *               +inf where there is none; c < C, C = 1 or 2.
 *   quantise    IEEE double, one rounding per operation: v = 1.0 - a / tau; q = 0 unless v > 0, else min(255, floor(256.0 v)).
 *               +inf and NaN ages give 0.  Q (K, C, h, w) uint8; Q is 0 off the sensor.
 *   cost        d = d_min + i, i = 0 .. nd - 1; 0 <= d_min, 1 <= nd <= 256, 1 <= radius <= 7.
 *               cost[k, i, y, x] = sum over c, |dy| <= r, |dx| <= r of |QL[k, c, y + dy, x + dx] - QR[k, c, y + dy, x + dx - d]|,
 *               an integer <= C (2 r + 1)^2 255.  d is admissible at x iff 0 <= x - d <= w - 1.
 *   candidate   max_c QL[k, c, y, x] >= min_activity (1 .. 255) and some d is admissible.
 *   winner      d* the admissible d of least cost, the smallest on ties; c1 its cost; c2 the least cost over admissible d with
 *               |d - d*| > 1, if there is one.
 *   tests       integer tests on a candidate, valid iff all pass:
 *               uniqueness u (0 .. 99): there is no c2, or c2 (100 - u) >= 100 c1;
 *               max cost: c1 <= max_cost (max_cost < 0: no test);
 *               left-right (lr_tolerance < 0: no test): x' = x - d*, dR the d with 0 <= x' + d <= w - 1 of least
 *               cost[k, d - d_min, y, x' + d], the smallest on ties; |dR - d*| <= lr_tolerance.
 *   sub-pixel   when d* - 1 and d* + 1 are in the range and admissible, with costs cm and cp and den = cm - 2 c1 + cp > 0:
 *               disparity = (float)((double)d* + (double)(cm - cp) / (double)(2 den)); else (float)d*.
 *   outputs     (K, h, w): index int32 d*, -1 where not valid; cost int32 c1, -1 where not a candidate; disparity float32, NaN
 *               where not valid; mask uint8.
 * Every cost is an integer and integer adds commute: the results are the same bits however the sums are tiled or ordered.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_STEREO_MAX_DISPARITIES 256
#define EVK_STEREO_MAX_RADIUS 7
/* ages: n device doubles; q: n bytes.  EVK_EINVAL, before any device work, for n < 0, tau not positive and finite, or a missing
 * pointer with n > 0. */
int evk_stereo_quantise(const double *ages, int64_t n, double tau, void *q, void *stream);
/* ql, qr: nk x nc x h x w device bytes; volume: nk x nd x h x w int32, -1 where d is not admissible.  EVK_EINVAL, before any
 * device work, for nk < 1, nc outside 1 .. 2, h < 1, w < 1, h w > 2^31 - 1, nk nd h w > 2^40, nd outside 1 .. 256, d_min outside
 * 0 .. 2^30, radius outside 1 .. 7 or a missing pointer. */
int evk_stereo_cost_volume(const void *ql, const void *qr, int nk, int nc, int h, int w, int d_min, int nd, int radius, void *volume,
                           void *stream);
/* The scratch of evk_stereo_match in bytes: 4 nk h w with a left-right test, 0 without; negative (EVK_EINVAL) for sizes the call
 * refuses. */
int64_t evk_stereo_scratch_bytes(int nk, int h, int w, int lr_tolerance);
/* As above; min_activity 1 .. 255, uniqueness 0 .. 99, max_cost and lr_tolerance negative for no test, subpixel 0 / 1; scratch:
 * evk_stereo_scratch_bytes(...) device bytes, any content (not read when that is 0).  Outputs nk x h x w each: disparity float32,
 * index int32, cost int32, mask uint8.  EVK_EINVAL, before any device work, for sizes as above, a parameter outside its range or a
 * missing pointer. */
int evk_stereo_match(const void *ql, const void *qr, int nk, int nc, int h, int w, int d_min, int nd, int radius, int min_activity,
                     int uniqueness, int64_t max_cost, int lr_tolerance, int subpixel, void *scratch, float *disparity, void *index,
                     void *cost, void *mask, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Semi-global matching (evk_sgm.hip): path aggregation of a stereo cost volume (Hirschmueller, PAMI 2008), and the winner of any
 * cost volume under the tests of "Event stereo".  All integers: the same bits every run.
 *
 *   input       volume (K, D, h, w) int32, 1 <= D <= 256, as evk_stereo_cost_volume writes it.  A cell is present iff its value
 *               is >= 0; a present cost counts as C = min(value, EVK_SGM_MAX_COST).  Presence is read from the sign, not from
 *               geometry: a volume with holes is legal, and a pixel may have no present cell at all.
 *   penalties   0 <= P1 <= P2 <= EVK_SGM_MAX_PENALTY.
 *   directions  r = (dx, dy), bit j of the mask: (1,0) (-1,0) (0,1) (0,-1) (1,1) (-1,-1) (1,-1) (-1,1).  At least one.
 *   path cost   for a pixel p, a direction r and q = p - r, for the present i of p: if q is off the sensor or has no present
 *               cell, L_r(p, i) = C(p, i).  Otherwise, with m = min_j L_r(q, j) over the present j of q,
 *               L_r(p, i) = C(p, i) + min( L_r(q, i), L_r(q, i - 1) + P1, L_r(q, i + 1) + P1, m + P2 ) - m,
 *               each of the first three terms only where that cell of q exists and is present.  C <= L_r <= C + P2.
 *   sum         S(p, i) = the sum over the chosen r of L_r(p, i) where the cell is present, -1 elsewhere; S <= 8 (2^22 + 2^20).
 *   winner      steps "candidate" to "outputs" of "Event stereo" on any (K, D, h, w) int32 volume with d = d_min + i: a cell is
 *               admissible iff its value is >= 0 and 0 <= x - d (there is no right pixel otherwise).  Candidates come from an
 *               activity surface (K, C, h, w) uint8; the tie rule, c2, the uniqueness test (its products in 64 bits), the
 *               left-right winner along volume[k, d - d_min, y, x' + d] and the parabola are as there; max_cost is an integer.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_SGM_MAX_COST 4194304
#define EVK_SGM_MAX_PENALTY 1048576
#define EVK_SGM_AGGREGATE 0
#define EVK_SGM_MATCH 1
/* The scratch of a call in bytes: EVK_SGM_AGGREGATE 8 nk nd h w (the d-contiguous copies of the costs and of the sums),
 * EVK_SGM_MATCH 4 nk h w; negative (EVK_EINVAL) for another call or sizes the calls refuse. */
int64_t evk_sgm_scratch_bytes(int call, int nk, int nd, int h, int w);
/* volume, out: nk x nd x h x w device int32 (out may be volume); directions: the mask above, 1 .. 255; scratch:
 * evk_sgm_scratch_bytes(EVK_SGM_AGGREGATE, ...) device bytes, any content.  EVK_EINVAL, before any device work, for nk < 1, h < 1,
 * w < 1, h w > 2^31 - 1, nk nd h w > 2^40, nk (h + w) > 2^31 - 1, nd outside 1 .. 256, penalties outside the range above or P1 > P2,
 * an empty or unknown direction mask, or a missing pointer. */
int evk_sgm_aggregate(const void *volume, int nk, int nd, int h, int w, int p1, int p2, int directions, void *scratch, void *out,
                      void *stream);
/* volume: nk x nd x h x w device int32; activity: nk x nc x h x w device bytes, nc 1 .. 2; d_min 0 .. 2^30; min_activity 1 .. 255,
 * uniqueness 0 .. 99, max_cost and lr_tolerance negative for no test, subpixel 0 / 1; scratch:
 * evk_sgm_scratch_bytes(EVK_SGM_MATCH, ...) device bytes, any content (not read without a left-right test).  Outputs nk x h x w each:
 * disparity float32, index int32, cost int32 (the winner's value in the volume), mask uint8.  EVK_EINVAL, before any device work, for
 * sizes as above, a parameter outside its range or a missing pointer. */
int evk_sgm_match_volume(const void *volume, const void *activity, int nk, int nc, int nd, int h, int w, int d_min, int min_activity,
                         int uniqueness, int64_t max_cost, int lr_tolerance, int subpixel, void *scratch, float *disparity, void *index,
                         void *cost, void *mask, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Camera tracking (evk_track.hip): 6-DoF registration of the semi-dense 3-D points of a reference view to a time surface, the
 * tracking step of ESVO (Zhou et al., T-RO 2021, section V).  The pose sought is the one under which the points project onto the
 * recent edges of the surface.
 *
 *   inputs      P (m, 3) doubles in the reference camera frame; fx, fy, cx, cy (no skew, undistorted); S (h, w) float32, low
 *               where events are recent; a pose (R, t), current-from-reference, as 12 doubles: R row-major, then t.
 *   per point   IEEE double, one rounding per operation, no transcendental function:
 *               X' = ((R00 Px + R01 Py) + R02 Pz) + tx, Y' and Z' likewise;  u = fx (X' / Z') + cx,  v = fy (Y' / Z') + cy.
 *               valid iff X', Y', Z' are finite, Z' > 0, 0 <= u < w - 1, 0 <= v < h - 1 and the four samples below are finite.
 *               x0 = floor(u), a = u - x0, a1 = 1 - a; y0, b, b1 likewise; S00 = S[y0, x0], S01 = S[y0, x0 + 1],
 *               S10 = S[y0 + 1, x0], S11 = S[y0 + 1, x0 + 1] as doubles.
 *               r  = b1 (a1 S00 + a S01) + b (a1 S10 + a S11)                   the bilinear value of S at (u, v)
 *               gx = b1 (S01 - S00) + b (S11 - S10),  gy = a1 (S10 - S00) + a (S11 - S01)     its exact derivative
 *               px = gx fx, py = gy fy;  j3 = (px / Z', py / Z', -((px X' + py Y') / (Z' Z')))
 *               J = (j3, X' x j3) = (j3, Y' j3_2 - Z' j3_1, Z' j3_0 - X' j3_2, X' j3_1 - Y' j3_0): the derivative of r for a left
 *               increment T <- exp(xi^) T, xi = (upsilon, omega).
 *   loss        EVK_TRACK_L2: w = 1, rho = r r.  EVK_TRACK_HUBER, delta > 0: w = 1 and rho = r r where |r| <= delta, else
 *               w = delta / |r| and rho = delta (2 |r| - delta).
 *   sums        over the valid points, 29 doubles per pose: A_ij = (w J_i) J_j for i <= j, row-major (21), g_i = (w J_i) r (6),
 *               c = rho, n = 1.  Summed by a fixed tree: a thread adds its 4 points (i = 1024 g + 256 q + t, q = 0 .. 3) in
 *               order, the 64 lanes of a wave are added by a scan on DPP, the 4 waves of a workgroup in order; of the
 *               ceil(m / 1024) workgroup rows, rows j, j + 8, j + 16, ... are added in order for j = 0 .. 7, then those eight in
 *               order.  The grid depends on m only; no floating-point atomics: a result is the same bits from run to run,
 *               and row b of a batch is the same bits as that pose alone.
 *   loop        evk_track_register: Levenberg-Marquardt on the host, one read-back of 29 doubles per evaluation.
 *               lambda = 1e-3.  Solve (A + lambda diag A) d = -g by Cholesky; the candidate is exp(d^) T; it is accepted iff
 *               n' >= min_points and c' / n' < c / n.  Accepted: lambda <- max(lambda / 10, 1e-9).  Rejected, or a failed
 *               Cholesky: lambda <- 10 lambda.  Ends when |d| < step_tol after an acceptance (EVK_TRACK_CONVERGED), lambda > 1e6
 *               (EVK_TRACK_STALLED), after max_evals evaluations (EVK_TRACK_MAX_EVALS), or at the start with n < min_points
 *               (EVK_TRACK_LOST).
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_TRACK_L2 0
#define EVK_TRACK_HUBER 1
#define EVK_TRACK_MAX_POSES 16
#define EVK_TRACK_SUMS 29
#define EVK_TRACK_CONVERGED 0
#define EVK_TRACK_STALLED 1
#define EVK_TRACK_MAX_EVALS 2
#define EVK_TRACK_LOST 3
/* The scratch of evk_track_terms and evk_track_register in bytes for m points and nb poses (the workgroup rows and one row of
 * sums per pose); negative (EVK_EINVAL) for m outside 1 .. 2^31 - 1 or nb outside 1 .. EVK_TRACK_MAX_POSES. */
int64_t evk_track_scratch_bytes(int64_t m, int nb);
/* points: m x 3 device doubles; surface: h x w device floats; poses: nb x 12 HOST doubles (they travel as kernel arguments);
 * scratch: evk_track_scratch_bytes(m, nb) device bytes, any content; sums: nb x 29 device doubles.  EVK_EINVAL, before any device
 * work, for a missing pointer, m outside 1 .. 2^31 - 1, h < 2, w < 2, h w > 2^31 - 1, nb outside 1 .. EVK_TRACK_MAX_POSES, a pose
 * or an intrinsic that is not finite, fx <= 0 or fy <= 0, another loss, or EVK_TRACK_HUBER with delta not positive and finite. */
int evk_track_terms(const double *points, int64_t m, const float *surface, int h, int w, double fx, double fy, double cx, double cy,
                    const double *poses, int nb, int loss, double delta, void *scratch, double *sums, void *stream);
/* The per-point values of one pose (12 HOST doubles) and no sums: r (m), jac (m x 6) device doubles, NaN where the point is not
 * valid; valid (m) device bytes 0 / 1.  EVK_EINVAL as above. */
int evk_track_residuals(const double *points, int64_t m, const float *surface, int h, int w, double fx, double fy, double cx,
                        double cy, const double *pose, double *r, double *jac, void *valid, void *stream);
/* The loop above from pose (12 HOST doubles, replaced by the result).  scratch: evk_track_scratch_bytes(m, 1).  Host results:
 * *cost = c and *n_valid = n at the returned pose, *evaluations, *status (EVK_TRACK_*).  Synchronises the stream once per
 * evaluation.  EVK_EINVAL as above, and for max_evals < 1, min_points < 1 or step_tol negative or NaN. */
int evk_track_register(const double *points, int64_t m, const float *surface, int h, int w, double fx, double fy, double cx, double cy,
                       double *pose, int loss, double delta, int max_evals, int64_t min_points, double step_tol, void *scratch,
                       double *cost, int64_t *n_valid, int *evaluations, int *status, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Depth fusion (evk_fusion.hip): inverse-depth maps with their variances carried through rigid motions into one view and fused
 * there, the map update of ESVO (Zhou et al., T-RO 2021, section IV-C) after the inverse-depth filters of LSD-SLAM (Engel et al.,
 * ECCV 2014), and the neighbourhood regularisation both apply afterwards.  Everything is an IEEE double with one rounding per
 * operation, in the order written here (the build sets -ffp-contract=off); no sqrt and no transcendental function;
 * tests/_fusion_np.py restates it in numpy.
 *
 *   map         (h, w): inv_depth rho and variance v doubles, NaN where there is nothing; count and rejected int32; mask bytes.
 *               A pixel is a source iff its mask is set and rho and v are finite and > 0; anything else is silently no source.
 *   view        s = 0 .. views - 1, 17 doubles each: fx, fy, cx, cy; R row-major, then t, target-from-source X' = R X + t; the
 *               process variance pv >= 0.  The target: fx', fy', cx', cy' and a size h' x w'.
 *   propagate   a source pixel (x, y) with (rho, v):
 *               Z = 1 / rho;  X = (((double)x - cx) / fx) Z;  Y = (((double)y - cy) / fy) Z
 *               X' = ((R00 X + R01 Y) + R02 Z) + t0, Y' and Z' likewise; dropped unless Z' > 0 and X', Y', Z' are finite
 *               rho' = 1 / Z';  u = fx' (X' / Z') + cx';  v_ = fy' (Y' / Z') + cy';  xi = floor(u + 0.5), yi = floor(v_ + 0.5);
 *               dropped unless 0 <= xi < w' and 0 <= yi < h' (compared as doubles, before the conversion to int32)
 *               q = rho' / rho;  q2 = q q;  v' = (q2 q2) v + pv; dropped unless v' is finite.
 *               (The variance rule of LSD-SLAM / ESVO: exact for a translation along the optical axis, where rho' / rho =
 *               1 / (1 + rho t_z); an approximation otherwise.)
 *   candidates  the surviving (xi, yi, rho', v'), ordered by view ascending, then by source pixel in row-major order.
 *   fuse        per target pixel, its candidates c_0 .. c_(m-1) in candidate order.  The anchor a is the one of least v', the
 *               earliest on ties.  Candidate i is an inlier iff i = a or, with d = rho'_i - rho'_a, d d <= gate2 (v'_i + v'_a);
 *               gate2 = gate gate, formed by the caller.  W = sum 1 / v'_i and S = sum rho'_i (1 / v'_i) over the inliers, one
 *               after the other in candidate order from 0.0.  inv_depth = S / W, variance = 1 / W, count = the inliers, rejected
 *               = m - count; m = 0: NaN, NaN, 0, 0.  mask = count >= min_count and (no max_variance or variance <= max_variance).
 *               An outlier of LOWER variance than the surface's candidates becomes the anchor and rejects them: the gate trusts
 *               the variances.  No occlusion reasoning (z-buffer) and no bilinear spreading over four pixels: out of scope.
 *   regularise  radius r in 1 .. EVK_FUSION_MAX_RADIUS.  For a masked pixel p, its compatible neighbours are the pixels q of
 *               the (2r+1)^2 window that lie inside the image, are masked and have (rho_q - rho_p)^2 <= gate2 (v_q + v_p); p
 *               itself is one (unless its own values fail the test: NaN).  n_p = their number without p.  inv_depth_out =
 *               (sum rho_q (1 / v_q)) / (sum 1 / v_q) over them in row-major window order from 0.0; mask_out = n_p >=
 *               min_neighbours.  A pixel that is not masked keeps its inv_depth, with the mask 0.  Variance, count and rejected
 *               are not touched: smoothing adds no information.
 * Pass structure: evk_fusion_propagate runs one thread per (view, source pixel), consecutive lanes on consecutive pixels,
 * stages a keep flag and the four columns in the scratch and compacts them in order (evk_select_compact, EVK_SELECT_FLAGS): the
 * order of the result is the candidate order.  The caller reads the count, groups the candidates by (xi, yi) with
 * evk_denoise_group (classes == 1, the same scratch: the staging is dead by then), and evk_fusion_fuse walks every pixel's run,
 * one lane per target pixel, twice: the anchor, then the sums.  The order of the sums is fixed, so a run is never split over
 * lanes: a pixel with many candidates makes one lane slow.  evk_fusion_regularise holds a 32 x 8 tile and its halo in LDS.  No
 * atomics: every result is the same bits from run to run.  The caller owns all memory; every call is ordered on `stream`.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_FUSION_MAX_RADIUS 3
#define EVK_FUSION_VIEW_PARAMS 17
/* The scratch of one fusion in bytes (256-byte aligned, any content): the larger of the staging of views h w (view, pixel) pairs
 * with its compaction (22 bytes each and the scratch of evk_select_compact) and the grouping of as many candidates on the out_h x
 * out_w plane (evk_denoise_scratch_bytes).  Negative (EVK_EINVAL) for a size below 1, views h w > 2^31 - 1 or out_h out_w >
 * 2^31 - 2, the limits of the grouping. */
int64_t evk_fusion_scratch_bytes(int views, int h, int w, int out_h, int out_w);
/* inv_depth, variance: views x h x w device doubles; mask: views x h x w device bytes; host_views: views x 17 HOST doubles and
 * host_target: 4 HOST doubles fx', fy', cx', cy' (they travel as kernel arguments, 16 views per launch); scratch:
 * evk_fusion_scratch_bytes(...) device bytes.  The candidate columns xi, yi (int32) and out_inv_depth, out_variance (doubles) hold
 * up to views h w elements; result: 3 device int64, the first the number of candidates (evk_select_compact).  EVK_EINVAL, before
 * any device work, for sizes as above, a missing pointer, a parameter that is not finite, fx, fy, fx' or fy' <= 0 or pv < 0;
 * EVK_EALIGN for a scratch that is not 256-byte aligned. */
int evk_fusion_propagate(const double *inv_depth, const double *variance, const void *mask, int views, int h, int w,
                         const double *host_views, int out_h, int out_w, const double *host_target, void *scratch, int32_t *xi,
                         int32_t *yi, double *out_inv_depth, double *out_variance, int64_t *result, void *stream);
/* On the grouping evk_denoise_group built in `scratch` from the m candidates' (xi, yi) on the out_h x out_w plane with classes ==
 * 1 (m = 0 included: its run table is all zeros); inv_depth, variance: their m device doubles (may be NULL when m = 0).  Outputs out_h x out_w each:
 * out_inv_depth, out_variance doubles, count, rejected int32, mask bytes 0 / 1.  EVK_EINVAL, before any device work, for a
 * missing pointer, m outside 0 .. 2^31 - 1, a plane the grouping refuses, gate2 negative or NaN, min_count < 1, use_max_variance
 * not 0 / 1 or a max_variance in use that is NaN. */
int evk_fusion_fuse(int64_t m, int out_h, int out_w, const void *scratch, const double *inv_depth, const double *variance, double gate2,
                    int min_count, int use_max_variance, double max_variance, double *out_inv_depth, double *out_variance,
                    int32_t *count, int32_t *rejected, void *mask, void *stream);
/* inv_depth, variance: h x w device doubles; mask: h x w device bytes; out_inv_depth (h x w doubles) and out_mask (h x w bytes)
 * must not be the inputs.  EVK_EINVAL, before any device work, for a missing or aliased pointer, h < 1, w < 1, h w > 2^31 - 1,
 * radius outside 1 .. EVK_FUSION_MAX_RADIUS, gate2 negative or NaN, min_neighbours outside 0 .. (2 radius + 1)^2. */
int evk_fusion_regularise(const double *inv_depth, const double *variance, const void *mask, int h, int w, int radius, double gate2,
                          int min_neighbours, double *out_inv_depth, void *out_mask, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Camera calibration (evk_camera.hip): lens undistortion and rectification of events and images, what the depth package above
 * takes as done.  No reference module.  Everything is an IEEE double with one rounding per operation, in the order written
 * here (the build sets -ffp-contract=off); tests/_camera_np.py restates it in numpy.
 *
 *   camera      K = (fx, fy, cx, cy), no skew, fx, fy > 0: pixel x = fx a + cx of the normalised coordinate a, a = (x - cx) / fx.
 *               Five coefficients d: EVK_CAMERA_RADTAN (k1, k2, p1, p2, k3); EVK_CAMERA_EQUIDISTANT (k1, k2, k3, k4, unused),
 *               Kannala-Brandt as Kalibr and OpenCV's fisheye model define it; EVK_CAMERA_NONE reads none.
 *   distort     (a, b) -> (a', b').
 *               radtan:  aa = a a, bb = b b, ab = a b, r2 = aa + bb;  rad = 1 + r2 (k1 + r2 (k2 + r2 k3));
 *                        dx = (2 p1) ab + p2 (r2 + 2 aa),  dy = p1 (r2 + 2 bb) + (2 p2) ab;  a' = a rad + dx,  b' = b rad + dy.
 *               equidistant:  r = sqrt(a a + b b), th = atan(r), thd(th) = th (1 + th2 (k1 + th2 (k2 + th2 (k3 + th2 k4)))) with
 *                        th2 = th th;  s = thd / r, and 1 where r < 1e-8;  a' = a s, b' = b s.
 *   undistort   (a', b') -> (a, b), exactly `iterations` steps with no early exit.
 *               radtan:  from (a, b) = (a', b'):  icd = 1 / rad(a, b);  (a, b) <- ((a' - dx(a, b)) icd, (b' - dy(a, b)) icd).
 *               equidistant:  rd = sqrt(a' a' + b' b'); from th = rd, Newton steps th <- th - (thd(th) - rd) / fp with
 *                        fp = 1 + th2 ((3 k1) + th2 ((5 k2) + th2 ((7 k3) + th2 (9 k4))));  s = tan(th) / rd, and 1 where
 *                        rd < 1e-8;  a = a' s, b = b' s.
 *               valid iff a and b are finite; for equidistant 0 <= th < pi / 2 (the nearest double); and with (ar, br) =
 *               distort(a, b): |fx (ar - a')| <= tolerance and |fy (br - b')| <= tolerance.  The fixed-point iteration diverges
 *               in the corners of a strongly distorted sensor: such a point is not valid.
 *   forward     EVK_CAMERA_FORWARD, raw pixel (x, y) -> rectified coordinate, for events:  (a, b) = undistort((x - cx) / fx,
 *               (y - cy) / fy);  X = (M00 a + M01 b) + M02, Y and Z likewise, M = R;  valid iff the undistortion is and Z > 0;
 *               u = fx' (X / Z) + cx', v = fy' (Y / Z) + cy'.
 *   inverse     EVK_CAMERA_INVERSE, rectified pixel (u, v) -> raw coordinate, for images, no iteration:  X, Y, Z as above from
 *               ((u - cx') / fx', (v - cy') / fy') with M = R^T;  (a', b') = distort(X / Z, Y / Z);  x = fx a' + cx,
 *               y = fy b' + cy;  valid iff Z > 0 and x and y are finite.
 *   A result that is not valid is NaN, its flag 0.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_CAMERA_NONE 0
#define EVK_CAMERA_RADTAN 1
#define EVK_CAMERA_EQUIDISTANT 2
#define EVK_CAMERA_FORWARD 0
#define EVK_CAMERA_INVERSE 1
#define EVK_CAMERA_NEAREST 0
#define EVK_CAMERA_SUBPIXEL 1     /* evk_camera_rectify_lookup */
#define EVK_CAMERA_BILINEAR 1     /* evk_camera_remap */
#define EVK_CAMERA_U8 0
#define EVK_CAMERA_F32 1
#define EVK_CAMERA_F64 2
/* n points through `direction`.  points: n interleaved (x, y) device doubles, or NULL: the points are the pixels of an h x w grid,
 * point i = (i mod w, i div w), and n must be h w (this is how both maps are built).  host_params: 22 HOST doubles (they travel
 * as a kernel argument): fx, fy, cx, cy; d[5]; M[9] row-major (R forward, R^T inverse); fx', fy', cx', cy'.  out: (2, n) device
 * doubles; valid: n device bytes 0 / 1.  EVK_EINVAL, before any device work, for another model or direction, fx, fy, fx' or fy' not
 * positive and finite, another parameter that is not finite, n, h or w negative, h w > 2^31 - 1, iterations < 1, tolerance negative
 * or NaN, a missing pointer.  n = 0: success, nothing is launched. */
int evk_camera_points(int model, int direction, const double *points, int64_t n, int h, int w, const double *host_params,
                      int iterations, double tolerance, double *out, void *valid, void *stream);
/* Events through a forward map.  x, y: n coordinates of kind coord_kind (EVK_SELECT_I16 .. F64), raw pixels.  map: (2, h, w) device
 * doubles; map_valid: h w device bytes 0 / 1.  With (u, v) the entry of pixel (x, y) and
 * `ok` its flag:
 *   EVK_CAMERA_NEAREST   (u, v) <- (rint(u) + 0, rint(v) + 0), halves to even, a negative zero becomes zero; keep iff ok and
 *                        0 <= u < out_w and 0 <= v < out_h.
 *   EVK_CAMERA_SUBPIXEL  keep iff ok and 0 <= u <= out_w - 1 and 0 <= v <= out_h - 1.
 * out_x, out_y: n values of kind out_kind, converted once from the doubles (a dropped event: 0); keep: n bytes 0 / 1, the flags
 * evk_select_compact(EVK_SELECT_FLAGS) takes.  A coordinate that is no integer, is NaN or is off the h x w sensor drops its event
 * and ORs 1 into the caller-zeroed *bad (may be NULL).  EVK_EINVAL for another kind or mode, a negative size, h w > 2^31 - 1, int16
 * outputs for more than 32768 columns or rows, a missing pointer.  n = 0: success, nothing is launched. */
int evk_camera_rectify_lookup(int coord_kind, const void *x, const void *y, int64_t n, const double *map, const void *map_valid, int h,
                              int w, int out_h, int out_w, int mode, int out_kind, void *out_x, void *out_y, void *keep, void *bad,
                              void *stream);
/* Image planes through an inverse map: src (planes, h, w) of dtype EVK_CAMERA_U8 / F32 / F64 -> dst (planes, out_h, out_w) of the
 * same dtype.  map: (2, out_h, out_w) device doubles (x, y on the raw sensor); map_valid as above.  F = fill rounded once to the
 * dtype (uint8: halves to even, then clamped to 0 .. 255).  With (mx, my) the entry of an output pixel, the pixel is F unless the
 * entry is valid and (rint(mx), rint(my)) is on the sensor; else
 *   EVK_CAMERA_NEAREST   src[rint(my), rint(mx)];
 *   EVK_CAMERA_BILINEAR  x0 = floor(mx), a = mx - x0, a1 = 1 - a; y0, b, b1 likewise; v00 = src[y0, x0], v01 = src[y0, x0 + 1],
 *                        v10 = src[y0 + 1, x0], v11 = src[y0 + 1, x0 + 1] as doubles, F where the tap is off the sensor;
 *                        b1 (a1 v00 + a v01) + b (a1 v10 + a v11), rounded once to the dtype as F is.
 * EVK_EINVAL for another dtype or interpolation, a negative size, h w or out_h out_w > 2^31 - 1, a missing pointer.  planes = 0 or
 * an empty output: success, nothing is launched. */
int evk_camera_remap(const void *src, int dtype, int64_t planes, int h, int w, const double *map, const void *map_valid, int out_h,
                     int out_w, int interpolation, double fill, void *dst, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Event augmentation (evk_augment.hip): lib/augmentation/event_augmentation.py's add_random_events (:60-92), remove_events
 * (:94-116) and add_correlated_events (:118-157).  Per-event random numbers: Philox4x32-10, key = the call's 64-bit seed,
 * counter = (index low word, index high word, purpose, 0); the purposes below.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_PHILOX_SUBSET 1        /* remove_events: the kept subset */
#define EVK_PHILOX_RANDOM_XY 2     /* random events: x (words 0-1), y (words 2-3) */
#define EVK_PHILOX_RANDOM_TP 3     /* random events: t (words 0-1), p (bit 0 of word 2) */
#define EVK_PHILOX_CORR_CHOICE 4   /* add_correlated_events: the chosen candidates */
#define EVK_PHILOX_CORR_XY 5       /* add_correlated_events: x, y jitter (one Box-Muller pair) */
#define EVK_PHILOX_CORR_T 6        /* add_correlated_events: t jitter */
/* out[4 i + w] = word w of Philox4x32-10 at counter (offset + i, purpose, 0), key seed (out 16-byte aligned) */
int evk_philox4x32(uint64_t seed, uint32_t purpose, uint64_t offset, int64_t n, uint32_t *out, void *stream);
/* bounds (4 device doubles) = {max x, max y, min t, max t} of n > 0 events (columns of EVK_SELECT_* kinds), each NaN when its
 * column holds a NaN (numpy's max / min).  scratch: evk_augment_bounds_scratch_bytes(). */
int64_t evk_augment_bounds_scratch_bytes(void);
int evk_augment_bounds(int kx, const void *x, int ky, const void *y, int kt, const void *t, int64_t n, double *bounds, void *scratch,
                       int64_t scratch_bytes, void *stream);
/* m random events from the bounds of evk_augment_bounds (read on the device): x uniform in [0, int(max x + 1)), y likewise, t
 * = min t + (max t - min t) * u with u a 53-bit uniform in [0, 1), p = +-1.  x, y, p are int64 (out_kind EVK_SELECT_I64) or
 * float64 (EVK_SELECT_F64); t float64.  Integers by 64-bit multiply-shift: bias below range / 2^64 (< 2^-32 for ranges below
 * 2^32).  A range numpy rejects gives 0: the caller checks the bounds. */
int evk_random_events(uint64_t seed, const double *bounds, int64_t m, int out_kind, void *x, void *y, double *t, void *p,
                      void *stream);
/* k jittered copies (float64): candidate sel[q] = c * n + e of event e: x[e] + trunc(xy_std * z), clipped to [0, max x], likewise
 * y, t[e] + ts_std * z, p[e]; z standard normals (Box-Muller in float64). */
int evk_correlated_events(uint64_t seed, const double *x, const double *y, const double *t, const double *p, int64_t n,
                          const int64_t *sel, int64_t k, double xy_std, double ts_std, const double *bounds, double *ox, double *oy,
                          double *ot, double *op, void *stream);
/* The float64 columns (x, y, t, p) in numpy's order of block.view('i8,i8,i8,i8').sort(order=['f2']): by the int64 bit patterns
 * of t, then x, y, p.  LSD radix sort of a permutation over the bit range in which each field varies (fields that do not vary
 * are skipped); *host_bits (may be NULL) receives the key bits sorted.  Synchronises the stream once (the bit ranges).
 * n < 2^31; scratch: evk_sort_events_scratch_bytes(n), 256-byte aligned. */
int64_t evk_sort_events_scratch_bytes(int64_t n);
int evk_sort_events_f64(const double *x, const double *y, const double *t, const double *p, int64_t n, double *ox, double *oy,
                        double *ot, double *op, void *scratch, int64_t scratch_bytes, int *host_bits, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Event-window datasets (lib/data_loaders/base_dataset.py): many voxel grids of one resident stream, RobustNorm
 * ---------------------------------------------------------------------------------------------------------- */
/* The voxel grids of nw windows [windows[2w], windows[2w+1]) of one stream in ONE launch (nw <= 65535), written to
 * vox = (nw, C, h, wd) float32, C = B (split = 0) or 2B (split = 1): every cell is written, no memset needed.
 *   x, y   xy_kind EVK_SELECT_I16 (int16) or EVK_SELECT_F32 (float32); xy_stride 2: one interleaved (N, 2) array in x
 *   t      EVK_T_F64 / EVK_T_F32;  p: EVK_P_U8_PM1 / EVK_P_U8 / EVK_P_I8 (one byte) or EVK_P_F32
 * Per window: t_i = (float)(t[i] - t[a_w]) with the subtraction in float64, dt = t_last - t_first in float32, then
 * events_to_voxel_torch's float32 arithmetic (voxel_grid.py:133-142): t_norm = t / dt * (B - 1),
 * w_b = p * max(0, 1 - |t_norm - b|) with NaN propagating (dt == 0 gives NaN cells, Q9), nearest pixel with the coordinate
 * truncated toward zero, a negative index wrapped once.  split: channels [0, B) weigh p > 0 ? 1 : 0, channels [B, 2B)
 * p <= 0 ? 1 : 0 (events_to_neg_pos_voxel_torch + torch.cat, base_dataset.py:451-453).  An empty window is one zero event
 * (base_dataset.py:218-223).  Events outside the grid are counted in *oob (the reference raises IndexError).  vox may have
 * any 4-byte alignment (16-byte aligned grids with h * wd a multiple of 4 are stored with 16-byte stores). */
int evk_voxel_windows_f32(const void *x, const void *y, int xy_kind, int xy_stride, const void *t, int t_kind, const void *p,
                          int p_kind, const int64_t *windows, int nw, int B, int h, int wd, int split, float *vox, uint32_t *oob,
                          void *stream);
/* return_events (base_dataset.py:306): rows [x, y, (float)(t - t[a_w]), p] of every non-empty window, window w from row
 * row_offsets[w] of the (rows, 4) float32 `out` (16-byte aligned).  Columns as for evk_voxel_windows_f32. */
int evk_pack_window_events_f32(const void *x, const void *y, int xy_kind, int xy_stride, const void *t, int t_kind,
                               const void *p, int p_kind, const int64_t *windows, const int64_t *row_offsets, int nw,
                               float *out, void *stream);
/* RobustNorm (data_augmentation.py:92-146) of n items of m = d0 * d1 * d2 float32 elements (m <= 2^31 - 4097): item i,
 * element (a, b, c) at x[i * item_stride + a * s0 + b * s1 + c * s2] (a CenterCrop view).  k_lo, k_hi: 1-based ranks of the
 * two percentiles (1 + round(.01 * q * (m - 1)), computed by the caller).  stats (n, 4) float32 receives per item the two
 * values in torch.kthvalue's order (NaN last, -0.0 and 0.0 tie), then min and max of the clamped item (NaN propagating).
 * out (n, m) contiguous: (clamp(x, lo, hi) - min) / (max + 1e-6) in float32; an item with lo == hi == 0 is copied unchanged.
 * Two launches: one workgroup per item selects, many per item write. */
int evk_robust_norm_f32(const float *x, int64_t n, int64_t item_stride, int d0, int d1, int d2, int64_t s0, int64_t s1,
                        int64_t s2, int64_t k_lo, int64_t k_hi, float *out, float *stats, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Raw event streams (evk_rawdecode.hip): Prophesee EVT3 / EVT2 words -> xs, ys, ts, ps columns.  The rules below
 * are this library's DEFINITION of the two formats; no vendor-written file has been decoded with it.
 *
 * EVT3: little-endian uint16 words, type = w >> 12.  State: y (11 bits), base_x (16 bits), vect_pol, t_low (12 bits), t_high
 * (12 bits), loops, have_time; all 0 / false at the start, or the caller's.
 *   0x0 ADDR_Y       y = w & 0x7FF (bit 11 ignored)
 *   0x2 ADDR_X       emits (w & 0x7FF, y, t, (w >> 11) & 1)
 *   0x3 VECT_BASE_X  base_x = w & 0x7FF, vect_pol = (w >> 11) & 1
 *   0x4 VECT_12      for each set bit i of w & 0xFFF, ascending, emits (base_x + i, y, t, vect_pol); then base_x += 12
 *   0x5 VECT_8       the same with w & 0xFF and base_x += 8
 *   0x6 TIME_LOW     t_low = w & 0xFFF
 *   0x8 TIME_HIGH    h = w & 0xFFF; if have_time and t_high - h >= 4085: loops += 1; else if have_time and t_high > h: counted
 *                    as time_went_back (and taken as it comes); t_high = h; have_time = true (t_low is kept)
 *   0xA EXT_TRIGGER  counted, not returned;  every other type: ignored, counted as `other`
 * t = (loops << 24) + (t_high << 12) + t_low microseconds.  A word that would emit while have_time is false emits nothing; its
 * events are counted as before_time.  base_x and base_x + i are 16-bit values (mod 2^16); x is stored as their int16 bits, so a
 * run of vectors that passes 32767 -- no sensor is that wide -- gives negative x, out of range for every sensor.
 * EVT2: little-endian uint32 words, type = w >> 28.  0x8 TIME_HIGH: t_high = w & 0x0FFFFFFF, have_time = true; 0x0 / 0x1
 * CD_OFF / CD_ON: emits (x = (w >> 11) & 0x7FF, y = w & 0x7FF, t = (t_high << 6) | ((w >> 22) & 0x3F), p = type); 0xA: a trigger;
 * the rest: other.  No loop handling (34-bit time), no time_went_back.
 *
 * state: 8 device int64 {y, base_x, vect_pol, t_low, t_high, loops, have_time, 0} (EVT2 uses t_high and have_time); fields
 * are masked to their widths on the way in.  result: 8 device int64 {events, triggers, other, before_time, time_went_back,
 * out_of_range, loops counted in this call, 0}.  Events come out in word order and bit order.
 *
 * Three launches, none of which waits for another workgroup: evk_raw_decode_plan reduces every chunk of EVK_RAW_CHUNK words to
 * an associative summary and combines the summaries in order behind state_in (one workgroup of EVK_RAW_SCAN_WIDTH lanes; with more
 * chunks than that a lane combines a run of consecutive chunks), writing result (out_of_range = 0) and state_out; the caller reads result[0], allocates the columns, and
 * evk_raw_decode_write -- same words, same scratch, untouched in between -- writes the events: xs, ys int16, ps uint8 {0, 1}, ts
 * int64 microseconds (EVK_RAW_TS_US) or float64 us / 1e6, one correctly rounded division (EVK_RAW_TS_SECONDS).  No position at
 * or behind result[0] is written, whatever the words hold.  sensor_h, sensor_w > 0: events with x >= sensor_w or y >= sensor_h
 * (unsigned 16-bit compares) are added to result[5]; they are written like the others.  flags: EVK_RAW_DIRECT_STORES -- every
 * lane stores its events itself instead of through a round of LDS staging (the A/B of profiles/raw_decode_time.txt).
 * words: aligned to its word size (an EVT3 column may start on any half word: a slice of an upload is read in place), n_words
 * <= EVK_RAW_MAX_WORDS.  state_in may be NULL (the initial state).  scratch: evk_raw_decode_scratch_bytes(n_words), 16-byte
 * aligned, any content.  The caller owns all memory; both calls are ordered on `stream`.
 * ---------------------------------------------------------------------------------------------------------- */
#define EVK_RAW_EVT3 3
#define EVK_RAW_EVT2 2
#define EVK_RAW_TS_US 0
#define EVK_RAW_TS_SECONDS 1
#define EVK_RAW_CHUNK 4096
#define EVK_RAW_SCAN_WIDTH 256
#define EVK_RAW_DIRECT_STORES 1
#define EVK_RAW_MAX_WORDS 0x10000000000
int64_t evk_raw_decode_scratch_bytes(int64_t n_words);
int evk_raw_decode_plan(const void *words, int64_t n_words, int format, const int64_t *state_in, void *scratch,
                        int64_t scratch_bytes, int64_t *result, int64_t *state_out, void *stream);
int evk_raw_decode_write(const void *words, int64_t n_words, int format, void *scratch, int64_t scratch_bytes, int64_t *result,
                         int16_t *xs, int16_t *ys, void *ts, uint8_t *ps, int ts_kind, int sensor_h, int sensor_w,
                         uint32_t flags, void *stream);

/* ------------------------------------------------------------------------------------------------------------
 * Event-sharded data parallelism: the path's only exchange step
 * Every accumulator is a sum over events (image.py:95,111-114,132-135: index_put_(accumulate=True); image.py:37:
 * np.bincount), so ranks holding disjoint event shards compute partial grids and ONE in-place SUM all-reduce of the grid
 * (voxel grid, IWE + dIWE buffer, integer event image) gives every rank the result.  These entry points wrap RCCL
 * (xGMI inside a node), bound at run time with dlopen: a process that already has an RCCL loaded (PyTorch) uses that
 * copy.  One process per GPU; rank 0 creates the id (evk_comm_unique_id_bytes() bytes), the application ships it to
 * the other ranks by whatever means it has (MPI, a file, torch.distributed), every rank calls evk_comm_init.
 * ---------------------------------------------------------------------------------------------------------- */
int evk_comm_unique_id_bytes(void);
int evk_comm_unique_id(void *host_id);
int evk_comm_init(const void *host_id, int rank, int world, void **comm_out);
int evk_comm_destroy(void *comm);
/* buf (device) <- sum over ranks of buf, enqueued on `stream`; int32 for the bit-exact integer event image */
int evk_allreduce_f32(float *buf, int64_t count, void *comm, void *stream);
int evk_allreduce_i32(int32_t *buf, int64_t count, void *comm, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EVK_H */
