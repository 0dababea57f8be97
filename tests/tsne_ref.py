"""Float64 numpy restatement of the t-SNE the svae_tsne_* kernels compute, written for this project's tests: the
perplexity calibration, the exact Student-t repulsion, the attraction over a directed k-NN graph (own edges plus the
scattered mirror force), van der Maaten's update and the whole fit. Every function also reports, where a test needs
it, the sum of the absolute values of the terms it added (the scale of a rounding-error bound)."""
import numpy as np


def blobs(N, Z, C, seed):
    """C Gaussian blobs in Z dimensions: centres ~ N(0, 18 I), unit-variance members, labels arange(N) % C."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((C, Z)) * np.sqrt(18.0)
    labels = np.arange(N) % C
    x = centres[labels] + rng.standard_normal((N, Z))
    return x.astype(np.float32), labels


def entropy64(p):
    p = np.asarray(p, np.float64)
    q = np.where(p > 0, p, 1.0)
    return -(p * np.log(q)).sum(-1)


def softmax64(dist, beta):
    """p_j = exp(-beta (d_j - d_min)) / sum, rows of dist [N, k], beta [N]."""
    d = np.asarray(dist, np.float64)
    x = d - d.min(-1, keepdims=True)
    e = np.exp(-np.asarray(beta, np.float64)[:, None] * x)
    return e / e.sum(-1, keepdims=True)


def affinities64(dist, perplexity, tol=1e-13, steps=400):
    """-> (p [N, k], beta [N]): per row the bisection on beta (start 1, double / halve while a bracket is open) until
    the entropy is within tol of log(perplexity)."""
    d = np.asarray(dist, np.float64)
    n, k = d.shape
    target = np.log(float(perplexity))
    p, betas = np.empty((n, k)), np.empty(n)
    for i in range(n):
        x = d[i] - d[i].min()
        beta, lo, hi = 1.0, -np.inf, np.inf
        for _ in range(steps):
            e = np.exp(-beta * x)
            s = e.sum()
            h = np.log(s) + beta * (x * e).sum() / s
            if abs(h - target) <= tol or not 1e-150 < beta < 1e150:   # degenerate rows never reach the target
                break
            if h > target:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else 0.5 * (beta + hi)
            else:
                hi = beta
                beta = beta * 0.5 if lo == -np.inf else 0.5 * (beta + lo)
        e = np.exp(-beta * x)
        p[i], betas[i] = e / e.sum(), beta
    return p, betas


def repulse64(y, chunk=512, with_abs=False, rows=None):
    """-> (rep [N, 2], zrow [N], zsum) with q = 1 / (1 + |y_i - y_j|^2), j != i excluded by index; with_abs: also the
    per-component sums of |q^2 (y_i - y_j)| [N, 2]. rows: only these rows i (against every j): the outputs have
    len(rows) rows and zsum is their sum alone."""
    y = np.asarray(y, np.float64)
    rows = np.arange(y.shape[0]) if rows is None else np.asarray(rows)
    n = len(rows)
    rep, zrow, arep = np.zeros((n, 2)), np.zeros(n), np.zeros((n, 2))
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        d = y[rows[c0:c1], None, :] - y[None, :, :]
        q = 1.0 / (1.0 + (d * d).sum(-1))
        q[np.arange(c1 - c0), rows[c0:c1]] = 0.0
        t = (q * q)[:, :, None] * d
        rep[c0:c1], zrow[c0:c1], arep[c0:c1] = t.sum(1), q.sum(1), np.abs(t).sum(1)
    out = (rep, zrow, zrow.sum())
    return out + (arep,) if with_abs else out


def attract64(y, nbr, p, with_abs=False):
    """-> attr [N, 2] = sum over the directed edges (i -> j = nbr[i][s], weight p[i][s]) of w q (y_i - y_j), added to
    row i, and its mirror -w q (y_i - y_j), added to row j; with_abs: also the sums of the terms' absolute values."""
    y = np.asarray(y, np.float64)
    nbr = np.asarray(nbr).astype(np.int64)
    n, k = nbr.shape
    src = np.repeat(np.arange(n), k)
    dst = nbr.reshape(-1)
    d = y[src] - y[dst]
    q = 1.0 / (1.0 + (d * d).sum(-1))
    f = (np.asarray(p, np.float64).reshape(-1) * q)[:, None] * d
    attr, aabs = np.zeros((n, 2)), np.zeros((n, 2))
    np.add.at(attr, src, f)
    np.add.at(attr, dst, -f)
    np.add.at(aabs, src, np.abs(f))
    np.add.at(aabs, dst, np.abs(f))
    return (attr, aabs) if with_abs else attr


def update64(y, vel, gains, attr, rep, zsum, N, exaggeration, learning_rate, momentum, inc=None):
    """One optimiser step -> (y, vel, gains, g). inc: the gains branch per coordinate (True: + 0.2, False: * 0.8);
    default: + 0.2 where vel and g have strictly opposite signs."""
    y, vel, gains, attr, rep = (np.asarray(a, np.float64) for a in (y, vel, gains, attr, rep))
    g = 4.0 * (float(exaggeration) / (2.0 * N) * attr - rep / float(zsum))
    if inc is None:
        inc = vel * g < 0.0
    gains = np.maximum(np.where(inc, gains + 0.2, gains * 0.8), 0.01)
    vel = float(momentum) * vel - float(learning_rate) * gains * g
    return y + vel, vel, gains, g


def fit64(dist, idx, init, n_iter, dtype=np.float64, perplexity=15.0, early_exaggeration=12.0, exaggeration_iter=250,
          learning_rate='auto', affinity_tol=1e-5, affinity_steps=100):
    """The whole fit from a k-NN graph, as the kernels are specified: the calibration stops where sklearn's does (the
    entropy within 1e-5 of its target, at most 100 steps), so beta walks the same dyadic bisection path here and on
    the device and the two sides embed the same affinities up to rounding. dtype float32: the same affinities
    (calibrated in float64, then cast) and every iteration's arithmetic in float32, for the noise floor of a float32
    implementation."""
    dt = np.dtype(dtype).type
    nbr = np.asarray(idx).astype(np.int64)
    n, k = nbr.shape
    p = affinities64(dist, perplexity, tol=affinity_tol, steps=affinity_steps)[0].astype(dt)
    lr = max(n / early_exaggeration / 4.0, 50.0) if learning_rate == 'auto' else float(learning_rate)
    y = np.array(init, dtype=dt)
    vel, gains = np.zeros_like(y), np.ones_like(y)
    src, dst = np.repeat(np.arange(n), k), nbr.reshape(-1)
    one = dt(1.0)
    for it in range(n_iter):
        early = it < exaggeration_iter
        ex, mom = dt(early_exaggeration if early else 1.0), dt(0.5 if early else 0.8)
        d = y[:, None, :] - y[None, :, :]
        q = one / (one + (d * d).sum(-1))
        np.fill_diagonal(q, 0)
        rep, zsum = ((q * q)[:, :, None] * d).sum(1), q.sum(dtype=dt)
        de = y[src] - y[dst]
        f = (p.reshape(-1) * q[src, dst])[:, None] * de
        attr = np.zeros_like(y)
        np.add.at(attr, src, f)
        np.add.at(attr, dst, -f)
        g = dt(4.0) * (ex / dt(2 * n) * attr - rep / zsum)
        gains = np.maximum(np.where(vel * g < 0, gains + dt(0.2), gains * dt(0.8)), dt(0.01))
        vel = mom * vel - dt(lr) * gains * g
        y = y + vel
        assert y.dtype == np.dtype(dtype)
    return y
