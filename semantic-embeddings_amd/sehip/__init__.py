"""sehip -- Python binding of libsehip.so, the MI355X (gfx950) kernels behind the cosine-embedding
training + retrieval hot path.  See include/sehip.h for the C ABI and DESIGN.md for the design."""
from ._lib import (DTYPE_BF16, DTYPE_F32, EXPORTS, LIB_PATH, METRIC_COSINE, METRIC_DOT, METRIC_EUCLID, SVM_GRAD, SVM_HV, SVM_SCORE, TOPK_MAX,
                   SehipError, build, lib)
from . import ops
from .ops import *  # noqa: F401,F403  -- every name of ops.__all__
