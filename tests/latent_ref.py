"""float64 restatement of the three latent-index scores (knn.py:28-50, math_utils.py:90-101 in the reference) and the
per-entry error bound the GPU tests hold the kernels to. Inputs are the f32 tensors the kernels read, promoted to
float64 here; nothing in this file runs product code."""
import numpy as np

METRICS = ('l2', 'cosine', 'kl')
LARGEST = {'l2': False, 'cosine': True, 'kl': False}
EPS24 = 2.0 ** -24


def random_posteriors(n, Z, seed, integer=False):
    """Seeded (mu, scale) f32 [n, Z]: scales log-uniform in [0.05, 2] (inv_var spans three decades); integer=True draws
    the means from the integers in [-8, 8] (every f32 L2 score is then exact, ties are plentiful)."""
    rng = np.random.default_rng(seed)
    if integer:
        mu = rng.integers(-8, 9, size=(n, Z)).astype(np.float32)
    else:
        mu = rng.standard_normal((n, Z)).astype(np.float32)
    scale = np.exp(rng.uniform(np.log(0.05), np.log(2.0), size=(n, Z))).astype(np.float32)
    return mu, scale


def scores64(metric, q_mu, q_scale, mu, scale):
    """-> (score [Q, N], A [Q, N]) in float64. A is the sum of the absolute values of the terms that make up the score
    (KL: |logdet_i| + |logdet_q| + Z / 2 + the quadratic terms; cosine: sum |mu_q mu_i| / (|mu_q| |mu_i|) + |score|)."""
    q_mu, q_scale, mu, scale = (np.asarray(a, dtype=np.float64) for a in (q_mu, q_scale, mu, scale))
    Z = mu.shape[1]
    if metric == 'l2':
        s = np.stack([((q - mu) ** 2).sum(-1) for q in q_mu])      # one query at a time: [N, Z] temporaries only
        return s, s.copy()
    if metric == 'cosine':
        nq = np.maximum(np.sqrt((q_mu ** 2).sum(-1)), 1e-8)
        ni = np.maximum(np.sqrt((mu ** 2).sum(-1)), 1e-8)
        den = nq[:, None] * ni[None, :]
        s = (q_mu @ mu.T) / den
        return s, (np.abs(q_mu) @ np.abs(mu).T) / den + np.abs(s)
    assert metric == 'kl'
    ld_q, ld_i = np.log(q_scale).sum(-1), np.log(scale).sum(-1)
    inv_var = 1.0 / scale ** 2
    quad = np.empty((q_mu.shape[0], mu.shape[0]))
    for q in range(q_mu.shape[0]):      # one query at a time: [N, Z] temporaries only
        quad[q] = ((q_scale[q] ** 2 + (q_mu[q] - mu) ** 2) * inv_var).sum(-1)
    s = (ld_i[None, :] - ld_q[:, None]) + 0.5 * quad - Z / 2
    return s, np.abs(ld_i)[None, :] + np.abs(ld_q)[:, None] + 0.5 * quad + Z / 2


def bound(A, Z):
    """|err| <= 4 (Z + 8) 2^-24 A: the f32 summation bound over Z + 8 operations, times 4 for the precomputed
    reciprocal and logf."""
    return 4.0 * (Z + 8) * EPS24 * A


def stable_topk(score_row, k, largest):
    """Indices of the best k of one row, ties to the lower index."""
    key = -score_row if largest else score_row
    return np.argsort(key, kind='stable')[:k]
