"""The policy networks the CPU and GPU tests share: the recorded ones (tests/golden/policy/policy_ref.npz, written by
tests/golden/make_golden_policy.py from the reference's own class) and the default width 256, whose weights would not fit a fixture
and are drawn here from a fixed seed.  Twin results are computed once per process and handed out read-only."""
import functools
import os

import numpy as np

from bunmpc_amd import policy

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "policy", "policy_ref.npz")
WIDE = (55, 256, 4, 12)


@functools.lru_cache(maxsize=None)
def recording():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@functools.lru_cache(maxsize=None)
def recorded(i):
    """(PolicyNet, x (16, in) float64, y (16, out) float32 of the reference's forward) of recorded net i"""
    r, k = recording(), "n%d_" % i
    sd = {str(key): r[k + "sd%d" % j] for j, key in enumerate(r[k + "keys"])}
    net = policy.PolicyNet.from_state_dict(sd, eps=float(r[k + "eps"]))
    assert net.dims == tuple(int(v) for v in r[k + "dims"])
    return net, r[k + "x"], r[k + "y"]


def n_recorded():
    return int(recording()["n_nets"])


def random_net(rng, n_in, hidden, layers, n_out, batch_norm=False):
    """Kaiming-scaled weights as the reference initialises them, biases of size 0.2"""
    K = [n_in] + [hidden] * layers
    N = [hidden] * layers + [n_out]
    W = [rng.normal(size=(n, k)) * np.sqrt(2.0 / k) for n, k in zip(N, K)]
    b = [rng.normal(size=n) * 0.2 for n in N]
    bn = [(rng.uniform(0.5, 1.5, hidden), rng.normal(size=hidden) * 0.3, rng.normal(size=hidden) * 0.5, rng.uniform(0.3, 2.5, hidden))
          for _ in range(layers)] if batch_norm else None
    return policy.PolicyNet.from_arrays(W, b, bn)


@functools.lru_cache(maxsize=None)
def wide_net():
    return random_net(np.random.default_rng(256), *WIDE)


def frozen(a):
    a.setflags(write=False)
    return a


def same_bits(got, want):
    """equal in every bit, NaN payloads aside: (n, w) arrays of one float type"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    bits = np.int64 if got.dtype == np.float64 else np.int32
    nan = np.isnan(got) & np.isnan(want)
    return bool(np.all((got.view(bits) == want.view(bits)) | nan))
