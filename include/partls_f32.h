/*
 * partls_f32.h — the float32 entry points of the C ABI of libpartls_hip.so.  Included by partls.h (include that, not this file): the
 * types, conventions and status codes are partls.h's, and these prototypes sit inside its extern "C" block.
 *
 * Why a header of its own: the ABI-consistency tests of the fp64 entry points (tests/test_abi.py, tests/test_julia_binding.py) parse
 * partls.h with symbol names without digits and a type map without `float *`.  They stay as they are, so these three prototypes and
 * their ctypes table (SYMBOLS_F32 in _lib.py) live beside partls.h, and tests/test_f32_binding.py applies the same header / library /
 * table / ccall checks to them.  Once those tests know `float *`, fold this file back into partls.h and SYMBOLS_F32 into SYMBOLS.
 */
#ifndef PARTLS_F32_H
#define PARTLS_F32_H
#ifndef PARTLS_H
#error "include partls.h, which includes this header"
#endif

/* ---- float32 design matrices: the same prepare for an X stored in single precision (the reference is generic over AbstractFloat and
 * its tests fit Float32 data, test/runtests.jl:123-146) --------------------------------------------------------------------------------
 * X: N x M floats, column-major, ldX in ELEMENTS (N <= ldX < 2^30); a host array, or with x_on_device a DEVICE array that stays owned by
 * the caller (a float32 torch tensor's data_ptr()).  X is uploaded, kept and read as float: half the PCIe bytes and half the HBM of the
 * widened copy (partls_get_upload reports 4 N M).  y, w (NULL: unweighted; rules of partls_opt_prepare_weighted) and every output stay
 * double: they are N numbers, the caller widens them.
 * Contract: every kernel that reads X widens each element to double as it loads it, which is exact (subnormals included), and all
 * arithmetic stays fp64 in the order of the fp64 path — so every result equals, bit for bit, that of partls_opt_prepare(_weighted) on
 * the widened matrix.  Only the storage and the transport of X change.
 * Every staged call then works as after the fp64 prepare: partls_opt_sweep, _finish, _pattern, _models, _candidates,
 * _merge_candidates, _bit_order, partls_alt_prepared, partls_bnb_prepared, partls_bnb_bound(_snap), partls_bnb_leaf, partls_bnb_search.
 * A float fit(Opt) is this + partls_opt_sweep + partls_opt_finish; fit(Alt) / fit(BnB) are this with PARTLS_OPT_FAITHFUL_INTERCEPT +
 * partls_alt_prepared / partls_bnb_prepared.  The next prepare of any kind decides the element type again.
 * Errors: those of the fp64 prepare (NaN / Inf in X -> PARTLS_ERR_NONFINITE, ldX < N -> PARTLS_ERR_BAD_ARG, ...).
 * Out of scope: a context of a partls_multi -> PARTLS_ERR_UNSUPPORTED (row-sharded multi-GPU fits stay fp64), and partls_cv_opt* has
 * no float form (widen on the host).  DESIGN.md §4.8. */
partls_status partls_opt_prepare_f32(partls_ctx *ctx, const float *X, int64_t N, int64_t M, int64_t ldX, const double *y,
                                     const double *w, int x_on_device, const int64_t *P, int64_t K, int64_t ldP, double eta,
                                     uint32_t flags);

/* The two predicts for a float X (N x M floats, ldX in elements; see partls_opt_prepare_f32): yhat / dyhat are doubles and equal
 * partls_predict(_device) on the widened matrix bit for bit. */
partls_status partls_predict_f32(partls_ctx *ctx, const float *X, int64_t N, int64_t M, int64_t ldX,
                                 const int64_t *P, int64_t K, int64_t ldP, const double *alpha, const double *beta, double t,
                                 double *yhat);
partls_status partls_predict_device_f32(partls_ctx *ctx, const float *dX, int64_t N, int64_t M, int64_t ldX,
                                        const int64_t *P, int64_t K, int64_t ldP, const double *alpha, const double *beta,
                                        double t, double *dyhat);

#endif
