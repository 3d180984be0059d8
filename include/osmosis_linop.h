/* osmosis_linop.h -- separable banded linear operators (blur, resampling) of libosmosis_hip.so: the second header of the
 * library's C ABI, beside osmosis_hip.h (whose conventions hold: 0 on success, a negative osm_status on failure with
 * osm_last_error() naming it, device pointers owned by the caller, `stream` a hipStream_t, NULL = default stream).
 * Strict C99.
 *
 * A = R_h (x) R_w per image plane, each factor a banded matrix given as a table: row i of R_h has its Kh non-zeros at the
 * columns start_h[i] .. start_h[i] + Kh - 1 with the values wt_h[i][0..Kh) (R_w alike).  Then
 *
 *   out[b * out_img_stride + p * Hout * Wout + i * Wout + j] =
 *       sum_a wt_h[i][a] * ( sum_c wt_w[j][c] * x[b * x_img_stride + p * Hin * Win + (start_h[i] + a) * Win + start_w[j] + c] )
 *
 * for b < B, p < P; the `zero_planes` planes that follow plane P - 1 of every output image are written as 0.  The image
 * strides (in elements) let the call read the colour planes of a [B,4,HW] tensor and write those of another.
 *
 * The transpose of a band is a band: the same call with the transposed tables is the exact adjoint.  Gather form: every
 * output element is written by exactly one lane; the horizontal sum is taken first, then the vertical one, taps ascending,
 * each tap one fp32 fused multiply-add -- no atomics, so the result depends on neither the launch shape nor the batch.
 * The tables live on the device and are the caller's to validate (0 <= start, start + K <= n_in); whatever they hold, a tap
 * that would read outside [0,Hin) x [0,Win) is skipped, never read. */
#ifndef OSMOSIS_LINOP_H
#define OSMOSIS_LINOP_H

#ifdef __cplusplus
extern "C" {
#endif

int osm_linop_apply(const float* x, float* out,
                    const int* start_h, const float* wt_h,   /* [Hout], [Hout][Kh] */
                    const int* start_w, const float* wt_w,   /* [Wout], [Wout][Kw] */
                    int B, int P, long long x_img_stride, long long out_img_stride,
                    int Hin, int Win, int Hout, int Wout, int Kh, int Kw,
                    int zero_planes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OSMOSIS_LINOP_H */
