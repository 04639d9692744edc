"""Golden fixture of the softmax classifier's loss: tests/golden/classifier_xent.npz.

CPU only, NumPy; runs where the reference checkout exists (oracle/ref_import.py).  The targets come from the reference's own
``learn_classifier.transform_inputs`` (learn_classifier.py:17-22: ``keras.utils.to_categorical`` + label smoothing); the loss is Keras
2.2's ``categorical_crossentropy`` on a softmax output, a third-party primitive restated here from its documented formula
(keras/backend/tensorflow_backend.py, ``categorical_crossentropy(target, output, from_logits=False)``):

    output /= sum(output, axis=-1, keepdims=True)
    output  = clip(output, epsilon, 1 - epsilon)            epsilon = 1e-7 cast to the output's dtype: the graph runs in float32, so
                                                            the bounds are float32(1e-7) and float32(1) - float32(1e-7) = 1 - 2^-23
    loss    = -sum(target * log(output), axis=-1)

with ``output = softmax(logits)`` = ``exp(z - max z) / sum exp(z - max z)`` (keras.activations.softmax).  Its gradient with respect
to the logits is the chain rule through exactly these steps (``clip`` passes gradient inside [epsilon, 1 - epsilon] only), evaluated
in float64.

Cases: logits N(0, scale^2) on a 1 / 32 grid (exact in float16, which keeps the file small; the coarse grid at scale 0.5 also produces
the ties the arg-max / top-k rules are about), B = 32 rows at C in {3, 10, 100, 1000} and B = 8 at C = 8142, scales 0.5 / 3 / 10,
smoothing 0 and 0.1.  Stored per case ``C{C}_x{scale}``: logits (float16), labels; per smoothing ``_s{0|1}``: loss64, loss32 (the
formula evaluated in float64 / float32) and grad64 for the first two rows at the columns ``gcols`` (all of them up to C = 1000, every
8th plus the labels' beyond).  ``flags`` is a JSON object: the flag names and defaults of the reference's command line
(learn_classifier.py:29-60 read from its source, utils.add_lr_schedule_arguments run on a real parser).

The tool asserts what the GPU test relies on: the float64 clamp form of include/sehip.h agrees with Keras' formula to 1e-13, and the
(row, class) pairs whose -log p lies within 2^-15 of the lower clip's threshold are at most 0.1 % of every case.

    python tools/make_classifier_golden.py
"""
import argparse
import ast
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
EPS32 = np.float32(1e-7)
ONE_MINUS_EPS32 = np.float32(1) - EPS32          # 1 - 2^-23
SHAPES = ((32, 3), (32, 10), (32, 100), (32, 1000), (8, 8142))
SCALES = (0.5, 3.0, 10.0)
SMOOTHINGS = (0.0, 0.1)


def softmax(z, fx):
    z = z.astype(fx)
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def keras_cce(Y, z, fx):
    """Keras 2.2 categorical_crossentropy(Y, softmax(z)) evaluated in ``fx``."""
    P = softmax(z, fx)
    P = P / P.sum(-1, keepdims=True)
    return -(Y.astype(fx) * np.log(np.clip(P, fx(EPS32), fx(ONE_MINUS_EPS32)))).sum(-1)


def keras_cce_grad(Y, z):
    """d keras_cce / d z in float64 by the chain rule: log <- clip <- renormalise <- softmax."""
    Y = Y.astype(np.float64)
    p = softmax(z, np.float64)
    S = p.sum(-1, keepdims=True)
    q = p / S
    inside = (q >= np.float64(EPS32)) & (q <= np.float64(ONE_MINUS_EPS32))
    dq = np.where(inside, -Y / q, 0.0)
    dp = dq / S - (dq * q).sum(-1, keepdims=True) / S
    return p * (dp - (dp * p).sum(-1, keepdims=True))


def clamp_form(Y, z):
    """The form of include/sehip.h (se_softmax_xent_fwd / _bwd) in float64."""
    Y, z = Y.astype(np.float64), z.astype(np.float64)
    m = z.max(-1, keepdims=True)
    lse = m + np.log(np.exp(z - m).sum(-1, keepdims=True))
    t = lse - z
    lo, hi = -np.log(np.float64(ONE_MINUS_EPS32)), -np.log(np.float64(EPS32))
    a = np.where((t >= lo) & (t <= hi), Y, 0.0)
    return (Y * np.clip(t, lo, hi)).sum(-1), a.sum(-1, keepdims=True) * np.exp(z - lse) - a, t, hi


def reference_flags():
    """{flag: default} of learn_classifier.py:29-60, from the add_argument calls of its source, plus the schedule flags."""
    src = open(os.path.join(ref_import.REFERENCE_ROOT, "learn_classifier.py")).read()
    flags = {}
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", None) == "add_argument":
            name = ast.literal_eval(node.args[0]).lstrip("-")
            kw = {k.arg: k.value for k in node.keywords}
            flags[name] = {"default": ast.literal_eval(kw["default"]) if "default" in kw else None,
                           "required": bool(ast.literal_eval(kw["required"])) if "required" in kw else False}
    sched = argparse.ArgumentParser()
    ref_import.import_reference("utils").add_lr_schedule_arguments(sched)
    for a in sched._actions:
        if a.dest != "help":
            flags[a.dest] = {"default": a.default, "required": False}
    return flags


def main():
    lc = ref_import.import_reference("learn_classifier", "float64")
    rng = np.random.default_rng(20181)
    out = {"flags": np.array(json.dumps(reference_flags(), sort_keys=True)), "smoothings": np.array(SMOOTHINGS),
           "cases": np.array(["C%d_x%g" % (C, sc) for _, C in SHAPES for sc in SCALES])}
    for B, C in SHAPES:
        for scale in SCALES:
            key = "C%d_x%g" % (C, scale)
            z = np.round(rng.standard_normal((B, C)) * scale * 32.0) / 32.0
            assert np.abs(z).max() < 64.0
            z16 = z.astype(np.float16)
            z = z16.astype(np.float32)
            y = rng.integers(0, C, size=B)
            gcols = np.arange(C) if C <= 1000 else np.unique(np.concatenate([np.arange(0, C, 8), y[:2]]))
            out[key + "_logits"], out[key + "_labels"], out[key + "_gcols"] = z16, y.astype(np.int64), gcols.astype(np.int32)
            for si, s in enumerate(SMOOTHINGS):
                _, Y = lc.transform_inputs(None, y, C, s)
                loss64, loss32 = keras_cce(Y, z, np.float64), keras_cce(Y, z, np.float32)
                grad64 = keras_cce_grad(Y, z)
                cl, cg, t, hi = clamp_form(Y, z)
                assert np.abs(cl - loss64).max() <= 1e-13 * max(1.0, np.abs(loss64).max()), (key, s)
                assert np.abs(cg - grad64).max() <= 1e-13, (key, s, np.abs(cg - grad64).max())
                window = (np.abs(t - hi) < 2.0 ** -15).mean()
                assert window <= 1e-3, (key, window)
                out["%s_s%d_loss64" % (key, si)], out["%s_s%d_loss32" % (key, si)] = loss64, loss32.astype(np.float32)
                out["%s_s%d_grad64" % (key, si)] = grad64[:2][:, gcols]
                print("%-12s s=%.1f  mean loss %.4f  clipped %.3f  window %.5f  |clamp - keras| %.1e  |f32 - f64| %.1e" % (
                    key, s, loss64.mean(), ((t > hi) | (t < -np.log(np.float64(ONE_MINUS_EPS32)))).mean(), window, np.abs(cl - loss64).max(),
                    np.abs(loss32 - loss64).max()))
    path = os.path.join(GOLDEN, "classifier_xent.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
