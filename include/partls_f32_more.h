/*
 * partls_f32_more.h — float32 entry points of the C ABI of libpartls_hip.so that came after the three of partls_f32.h.  Included by
 * partls.h (include that, not this file): the types, conventions and status codes are partls.h's, and these prototypes sit inside its
 * extern "C" block.
 *
 * Why a second header: tests/test_f32_binding.py pins the prototypes of partls_f32.h and the ctypes table SYMBOLS_F32 to exactly the
 * three entry points of the float32 design-matrix work, and tests/test_abi.py reads partls.h with symbol names without digits.  Those
 * tests stay as they are, so a later float32 entry point is declared here and bound in SYMBOLS_F32_MORE (_lib.py);
 * tests/test_predict_many_binding.py applies the header / library / table / ccall checks to it.  Fold both float32 headers back into
 * partls.h together (see partls_f32.h).
 */
#ifndef PARTLS_F32_MORE_H
#define PARTLS_F32_MORE_H
#ifndef PARTLS_H
#error "include partls.h, which includes this header"
#endif

/* partls_predict_many for a float X (N x M floats, ldX in elements; host, or with x_on_device a device array; see
 * partls_opt_prepare_f32): every output is double and equals partls_predict_many on the widened matrix bit for bit. */
partls_status partls_predict_many_f32(partls_ctx *ctx, const float *X, int64_t N, int64_t M, int64_t ldX, int x_on_device,
                                      const int64_t *P, int64_t K, int64_t ldP, int64_t B, const double *alpha, const double *beta,
                                      const double *t, double *yhat, int64_t ldY, int64_t nr, const int64_t *ranks, double *stats,
                                      double *mean);

#endif
