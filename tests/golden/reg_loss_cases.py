"""Seeded INPUTS of the RegistrationLoss fixture (reg_loss.npz, reg_loss_grads.npz): every case is regenerated from its numpy
seed here; the fixture stores only what the reference answered.  Imported by tests/golden/make_golden_loss.py (runs the
reference in fp32 and fp64), by the tests and by scripts/reg_loss_bench.py.  No reference code here."""
from types import SimpleNamespace

import numpy as np

TAU, EPS = 0.1, 0.5


def cfg(offset_value="manhattan", lambda_p=1.0, lambda_c=1.0, lambda_o=1.0, tau=TAU, eps=EPS):
    """the reference's `args` (RegistrationLoss reads args.loss.<key> for exactly these keys)"""
    return SimpleNamespace(loss=SimpleNamespace(tau=tau, offset_value=offset_value, eps_positive=eps, eps_offset=2.0,
                                                lambda_p=lambda_p, lambda_c=lambda_c, lambda_o=lambda_o))


def _make(seed, B, S, D, C=256, C2=128, side=3.0, overlap=0.6, noise=0.15, pad_s=0, pad_d=0, K=40, K2=33):
    """src uniform in a cube of `side`; the first overlap*D dst points are src points moved by up to `noise` per axis, the rest
    uniform; dst features of those points follow their src point's features (so the top-1 accuracy is not trivially 0)."""
    rng = np.random.default_rng(seed)
    xs = rng.uniform(0, side, (B, 3, S))
    xd = rng.uniform(0, side, (B, 3, D))
    fs = rng.standard_normal((B, C, S))
    fd = rng.standard_normal((B, C, D))
    cs = rng.standard_normal((B, C2, S))
    cd = rng.standard_normal((B, C2, D))
    n = min(int(overlap * D), S)
    for b in range(B):
        src = rng.permutation(S)[:n]
        xd[b, :, :n] = xs[b, :, src].T + rng.uniform(-noise, noise, (3, n))
        fd[b, :, :n] = fs[b, :, src].T + 0.7 * rng.standard_normal((C, n))
        cd[b, :, :n] = cs[b, :, src].T + 0.7 * rng.standard_normal((C2, n))
    ps = np.zeros((B, S), bool)
    pd = np.zeros((B, D), bool)
    if pad_s:
        ps[:, S - pad_s:] = True
    if pad_d:
        pd[:, D - pad_d:] = True
    return dict(xs=xs, xd=xd, ps=ps, pd=pd, fs=fs, fd=fd, cs=cs, cd=cd, os=rng.standard_normal((K, 3, 1)),
                od=rng.standard_normal((K2, 3, 1)))


ULP_EPS = 0.3   # not a binary fraction: fp32(eps)^2 and fp32(eps^2) differ in the last bits


def _ulp_case(seed):
    """src points at x = 0, their dst partners at x = fp32(eps) and the three fp32 neighbours either side of it: the fp32
    threshold rule (dist2 <= fp32(eps^2)) decides which are corr; nothing else lies within eps."""
    c = _make(seed, 1, 14, 14, side=30.0, overlap=0.0)
    e = np.float32(ULP_EPS)
    steps = [e]
    for _ in range(3):
        steps = [np.nextafter(steps[0], np.float32(0))] + steps + [np.nextafter(steps[-1], np.float32(1))]
    for k in range(14):
        c["xd"][0, :, k] = c["xs"][0, :, k]
        c["xs"][0, 0, k] = 0.0
        c["xd"][0, 0, k] = steps[k % 7]
    return c


def cases():
    """name -> (inputs dict of float64 / bool arrays, cfg, grads recorded?).  Coordinates are rounded to fp32 first, so the
    fp64 run sees the same points."""
    out = {}

    def add(name, inputs, c, grads=False):
        for k in ("xs", "xd"):
            inputs[k] = inputs[k].astype(np.float32).astype(np.float64)
        out[name] = (inputs, c, grads)

    add("padding_both", _make(1, 2, 96, 80, pad_s=9, pad_d=13), cfg("manhattan"), grads=True)
    add("s_ne_d_lambda", _make(2, 2, 60, 68), cfg("euclidean", lambda_p=0.7, lambda_c=1.9, lambda_o=0.35), grads=True)
    add("multi_tile", _make(3, 2, 333, 520, side=6.0, pad_s=17, pad_d=30), cfg("mahalanobis"))
    add("s1_d1", _make(4, 1, 1, 1, side=0.1, K=1, K2=1), cfg("manhattan"))
    add("s1_d1_far", _make(5, 1, 1, 1, side=100.0, overlap=0.0, K=0, K2=2), cfg("euclidean"))
    c = _make(6, 2, 50, 40, side=30.0)
    c["pd"][:, :24] = True                        # the dst points that have a src partner are padding: dst -> src has no rows
    add("no_pos_dst", c, cfg("euclidean"))
    add("no_pos_both", _make(7, 2, 30, 20, side=100.0, overlap=0.0), cfg("mahalanobis"))
    add("all_neutral", _make(8, 2, 24, 20, side=0.2, overlap=1.0, noise=0.01), cfg("manhattan"))
    c = _make(9, 2, 70, 64, side=2.0)
    c["xd"][:, :, 32:64] = c["xd"][:, :, 0:32]      # duplicated dst points: the nearest neighbour ties (first index wins)
    add("dup_dst", c, cfg("manhattan"))
    add("ulp_eps", _ulp_case(10), cfg("euclidean", eps=ULP_EPS))
    return out


def mask_tolerance_cases():
    """the cases whose fp64 masks must equal the fp32 ones (the generator asserts it): all but the one built on the threshold"""
    return [k for k in cases() if k != "ulp_eps"]
