"""MI355X-native Partitioned Least Squares — host-side mirror of PartitionedLS.jl's interface for the hot path.

    from partls_amd import package; pls = package()
    model, _, report = pls.fit(pls.Opt, X, y, P, η=0.0)          # Opt.jl:73
    yhat = pls.predict(model, X)                                  # PartitionedLS.jl:152

Same names, argument meaning and result layout as the reference's exported API (PartitionedLS.jl:3):
fit, predict, PartLSFitResult, Opt, Alt, BnB, homogeneousCoords, regularizeProblem.
All arithmetic runs in libpartls_hip.so (hand-written HIP for gfx950) through the C ABI of include/partls.h;
there is no CPU fallback — importing works anywhere, computing needs an MI355X and raises otherwise.
"""
from .api import (Alt, BnB, BootstrapResult, CSR, CVResult, Context, Diagnostics, Frontier, IllConditionedWarning, MultiContext, Opt, PartLSFitResult, PartlsError, Report, TopPatterns, bootstrap, build_library, contributions, contributions_many, cross_validate, cv_folds, default_context, diagnostics, default_multi, fit, fit_robust, RobustConvergenceWarning, fit_glm, predict_mean, GLMConvergenceWarning,
                  group_importance, homogeneousCoords, library_path, predict, predict_device, predict_many, regularizeProblem, resample, synth_truth)
from . import _lib as lowlevel
from . import dist

__all__ = ["fit", "predict", "PartLSFitResult", "Opt", "Alt", "BnB", "homogeneousCoords", "regularizeProblem",
           "PartlsError", "IllConditionedWarning", "Report", "build_library", "library_path", "lowlevel", "Context", "Frontier", "MultiContext", "default_context", "default_multi", "synth_truth", "dist", "predict_device", "cross_validate", "cv_folds", "CVResult", "bootstrap", "resample", "BootstrapResult", "predict_many", "TopPatterns", "CSR", "contributions", "contributions_many", "group_importance", "diagnostics", "Diagnostics", "fit_robust", "RobustConvergenceWarning", "fit_glm", "predict_mean", "GLMConvergenceWarning"]
