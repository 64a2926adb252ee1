"""The band of the packed nearest-cell keys (csrc/swarm_env.hip, nearest_rows_lean and the `tol` behind it), on the host.

The N = 64 lattice kernels keep best and runner-up of the nearest-cell walk as (bits of d2 & ~7) | candidate number, so the
two distances reach the test `second - best <= tol` without their last three mantissa bits, and the candidate that leads is
only the first of those that agree in the kept bits.  The kernel adds `tol_keys = K * second32` to the band
tol = 6 sqrt(second32) lat_dlt + 1e-9 for it.  Two properties make that sound, for any non-negative fp32 best <= second
and any lat_dlt the kernel can form:

  sent   a lane that the full-width test sends to the exact scan is still sent: second - best <= tol(second) implies
         trunc(second) - trunc(best) <= tol(trunc(second)) + K trunc(second);
  thr    the exact scan's threshold is no lower, and it reaches every candidate that agrees with the leader in the kept bits:
         trunc(best) + tol(trunc(second)) + K trunc(second) >= best + tol(second), and >= trunc(best) + 8 ulp(best).

K is read from the kernel's source, so the term cannot go or shrink unnoticed; the same checks with K = 0 must fail, or
they would hold nothing.  All arithmetic is numpy float32, as the kernel's.
"""
import os
import re

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "marl_llm_amd", "csrc", "swarm_env.hip")
f32 = np.float32


def key_term():
    """K of `tol_keys = K * second32` in the kernel's source, a hexadecimal float."""
    m = re.search(r"tol_keys = (0x1p-\d+)f \* second32;", open(SRC).read())
    assert m, "the band term of the packed keys is not in the source"
    return f32(float.fromhex(m.group(1)))


def trunc(x):
    return (x.view(np.uint32) & np.uint32(0xFFFFFFF8)).view(np.float32)


def tol(second, dlt):
    return f32(6.0) * np.sqrt(second) * dlt + f32(1e-9)


def samples(n=400000, seed=0):
    """best <= second over thirteen octaves of squared steps (1/64 .. 128 steps), the pair up to 64 ulp apart or far apart,
    lat_dlt from its floor (2e-6) to that of coordinates of 128 steps."""
    rng = np.random.default_rng(seed)
    best = np.exp2(rng.uniform(-12, 14, n)).astype(f32)
    gap = np.where(rng.random(n) < 0.7, rng.integers(0, 64, n), rng.integers(0, 1 << 20, n)).astype(np.uint32)
    second = (best.view(np.uint32) + gap).view(np.float32)
    dlt = (f32(1.2e-7) * rng.uniform(0, 128, n).astype(f32) + f32(2e-6)).astype(f32)
    return best, second, dlt


def violations(K):
    best, second, dlt = samples()
    bt, st = trunc(best), trunc(second)
    band = tol(st, dlt) + K * st
    sent_full = (second - best) <= tol(second, dlt)
    sent = (st - bt) <= band
    ulp8 = (np.spacing(best) * f32(8)).astype(f32)
    thr_ok = (bt.astype(np.float64) + band >= best.astype(np.float64) + tol(second, dlt)) & (bt.astype(np.float64) + band >= bt.astype(np.float64) + ulp8)
    return int((sent_full & ~sent).sum()), int((sent_full & ~thr_ok).sum())


def test_band_covers_the_bits_the_keys_give_up():
    K = key_term()
    assert K == f32(2.0 ** -19)
    assert violations(K) == (0, 0)


def test_without_the_term_the_band_is_too_narrow():
    lost, low = violations(f32(0))
    assert lost > 0 and low > 0, (lost, low)


def test_keys_order_like_the_distances_and_the_sentinels_stay_on_top():
    """Non-negative floats order like their bits; a sentinel candidate (>= 1.8e19), kNoCand (1e18) and +inf stay above every
    real candidate after the truncation, whatever the candidate number in the low bits."""
    rng = np.random.default_rng(1)
    d = np.sort(np.exp2(rng.uniform(-20, 40, 10000)).astype(f32))
    keys = (d.view(np.uint32) & np.uint32(0xFFFFFFF8)) | rng.integers(0, 8, d.size).astype(np.uint32)
    assert (np.diff((keys & np.uint32(0xFFFFFFF8)).astype(np.int64)) >= 0).all()
    real = (f32(1e12).view(np.uint32) & np.uint32(0xFFFFFFF8)) | np.uint32(7)          # (128 steps)^2 is 1.6e4: far below
    assert f32(1e18).view(np.uint32) > real
    for top in (f32(1.8e19), f32(np.inf)):                          # what a side without a column and an unseen runner-up hold
        assert (top.view(np.uint32) & np.uint32(0xFFFFFFF8)) > real
        assert trunc(np.array([top]))[0] >= f32(1e18)               # still "no candidate" to the caller's test against kNoCand
