"""Data of the power-of-two scale tests (tests/test_oracle_cpu.py, tests/test_knn_scale_gpu.py).

Every component has a magnitude in [2^-3, 4] (up to a relative 2^-12) and a random sign, so that x * 2^s stays a normal fp32
number for |s| <= 120: scaling by a power of two then commutes with every fp32 and bf16 rounding, and
  inner product  (X 2^s, Q 2^-s)  gives the same products q_i x_i, hence bit-identical D and I;
  L2             (X 2^s, Q 2^s)   gives D 4^s and the same I while ||q||^2 + ||x||^2 stays a normal number;
  "L2norm,"      either way       gives bit-identical normalised rows while the squared norms stay normal numbers.
Near-ties are planted where the k-th neighbour is decided: each query is a jittered copy of one of a few base rows, and every
base row has `clones` copies in X that differ from it by at most 2^-12 relative per component -- below bf16's resolution, so the
bf16 scores of a base's clones mostly tie while their exact scores differ."""
import numpy as np

IP_SWEEP = (-100, -70, -66, -64, -40, 0, 40, 62, 64, 66, 70, 100)
L2_SWEEP = (-40, -20, 20, 40, 50, 55)
L2NORM_SWEEP = (-55, -40, 40, 55)  # ||x||^2 stays normal for d <= 1024: 2^-6 4^s >= 2^-126 and 2^4 d 4^s (1 + 2^-11) < 2^128


def components(rng, shape):
    mag = np.exp2(rng.uniform(-3.0, 2.0, shape))
    return (mag * rng.choice((-1.0, 1.0), shape)).astype(np.float32)


def planted(seed, n, d, nq, clones, bases=8, query_jitter=2.0 ** -6, return_rows=False):
    """(X [n, d], Q [nq, d]) float32: `bases` base rows with `clones` near-copies each, scattered over X; query j is base
    j % bases with every magnitude jittered by up to `query_jitter` relative (same signs).  return_rows: + the [bases, clones]
    row numbers of the copies."""
    rng = np.random.default_rng(seed)
    assert bases * clones <= n
    X = components(rng, (n, d)).astype(np.float64)
    base = components(rng, (bases, d)).astype(np.float64)
    rows = rng.permutation(n)[:bases * clones].reshape(bases, clones)
    for b in range(bases):
        X[rows[b]] = base[b] * (1.0 + rng.uniform(-2.0 ** -12, 2.0 ** -12, (clones, d)))
    Q = base[np.arange(nq) % bases] * (1.0 + rng.uniform(-query_jitter, query_jitter, (nq, d)))
    if return_rows:
        return X.astype(np.float32), Q.astype(np.float32), rows
    return X.astype(np.float32), Q.astype(np.float32)


def scaled(a, s):
    """a * 2^s, exactly (every element stays normal for the data above and |s| <= 120)."""
    return np.ldexp(np.asarray(a, dtype=np.float32), s).astype(np.float32)
