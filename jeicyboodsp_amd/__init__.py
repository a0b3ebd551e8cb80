"""jeicyboodsp_amd -- MI355X (gfx950) engine for JeicybooDSP's FFT-based spectral
path.  The product is libjdsp.so (hand-written HIP kernels behind the C ABI in
include/jdsp.h); this package is the thin Python mirror used by tests and
bench.py.  PyTorch is used only to own device memory and streams."""
from ._lib import JdspError, LIB_PATH  # noqa: F401
from .engine import (GMM_PARAM, GMM_TRAIN_PARAM, GMM_TRAIN_STATS, HMM_PARAM, Denoiser, Engine, FastConv, Geq, Gmm,  # noqa: F401
                     GmmTrainer, Hmm, Mfcc, Mvdr, MvdrMulti, Nlms, geq_design, to_score_params)

__all__ = ["Engine", "Denoiser", "FastConv", "Mfcc", "Mvdr", "MvdrMulti", "Gmm", "Hmm", "GMM_PARAM", "HMM_PARAM",
           "GmmTrainer", "GMM_TRAIN_PARAM", "GMM_TRAIN_STATS", "to_score_params", "Geq", "Nlms", "geq_design",
           "JdspError", "LIB_PATH"]
