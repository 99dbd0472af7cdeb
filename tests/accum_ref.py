"""Restatement of the gradient-accumulation launch (csrc/adam.hip grad_accum_multi_kernel, csrc/adam_update.h) in numpy
float32:  acc = beta acc + w g  with the two products and the sum each rounded to float32 (numpy rounds every float32
operation; nothing here can contract into an fma), and at beta == 0  acc = w g  without reading the accumulator.
optim.FusedAdam.accumulate(weight, first) is beta = 0 if first else 1, w = float32(weight)."""
import numpy as np


def accumulate(acc, g, beta, w):
    """One launch on one tensor: acc (float32 array, or anything at beta == 0), g (float32 array) -> the new acc."""
    f = np.float32
    g, beta, w = np.asarray(g, dtype=f), f(beta), f(w)
    if beta == f(0.0):
        return w * g
    return beta * np.asarray(acc, dtype=f) + w * g


def accumulate_all(micro_grads, weights):
    """micro_grads: per micro-batch, a list of float32 arrays (one per parameter); weights: one per micro-batch
    -> the accumulated gradient per parameter after the last micro-batch (first launch beta = 0, then beta = 1)."""
    acc = [None] * len(micro_grads[0])
    for m, (gs, w) in enumerate(zip(micro_grads, weights)):
        acc = [accumulate(a, g, 0.0 if m == 0 else 1.0, w) for a, g in zip(acc, gs)]
    return acc
