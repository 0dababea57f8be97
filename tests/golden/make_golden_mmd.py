"""Generate tests/golden/mmd.npz: inputs and the outputs of the reference's three MMD estimators
(sparse_vae/core/math_utils.py:104-184), run on the CPU in float64 (the expected values) and in float32 (for the
record: the reference's own f32 run differs from its f64 run in the third or fourth digit).

    python tests/golden/make_golden_mmd.py REFERENCE_ROOT      (the checkout that holds sparse_vae/core/math_utils.py)

The reference module is loaded by path at generation time only; nothing of it is copied. Inputs are f32:
  a   N(0, I) at (513, 16)        b   N(0, I) at (300, 64)
  a_shrunk, b_shrunk   0.5 * the above        a_shift, b_shift   the above + 30 in every coordinate
  prior16, prior16_pair   the two sets of 1000 standardised prior samples gaussian_imq_mmd_sq draws for Z = 16 after
            torch.manual_seed(PRIOR_SEED): the first for its cross term, the second for its prior-prior term (its two
            helpers call the cached sampler with different argument lists, so the cache holds two draws)
Outputs, per input name X: X/analytic_std, X/analytic_raw, X/custom_std, X/custom_raw (against the diagonal Gaussian
of X/mean, X/var: the input's own column mean and unbiased variance, rounded to f32), and for the Z = 16 inputs
X/imq; each also as X/..._f32.
The IMQ cases satisfy min over scales and pairs of (s + d2 + offset) >= 1 (asserted below): the reference divides by
that quantity, and its cross term's |x|^2 - 2 x.p + Z can be negative."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mmd_ref  # noqa: E402

# chosen for the condition above: with most seeds some pair of the N(0, I) input has |x|^2 - 2 x.p + Z < 1 - s_min
# (about one seed in 28 of 0..1999 meets it; this one leaves the widest margin of the first 1000)
PRIOR_SEED = 502


def load_reference(root):
    spec = importlib.util.spec_from_file_location('ref_math_utils',
                                                  os.path.join(root, 'sparse_vae', 'core', 'math_utils.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('reference', help='root of the reference checkout')
    args = ap.parse_args()
    ref = load_reference(args.reference)
    rng = np.random.default_rng(20240)
    base = {'a': rng.standard_normal((513, 16)).astype(np.float32),
            'b': rng.standard_normal((300, 64)).astype(np.float32)}
    inputs = {}
    for k, v in base.items():
        inputs[k] = v
        inputs[k + '_shrunk'] = (np.float32(0.5) * v).astype(np.float32)
        inputs[k + '_shift'] = (v + np.float32(30.0)).astype(np.float32)
    # the samples the reference's IMQ draws after this seed (its helper is a closure: the same generator call here)
    torch.manual_seed(PRIOR_SEED)
    draws = []
    for _ in range(2):
        raw = torch.randn(1000, 16)
        var, mean = torch.var_mean(raw)
        draws.append(((raw - mean) / var.sqrt()).numpy())
    prior = draws[0]
    out = {'prior16': prior, 'prior16_pair': draws[1], 'prior_seed': np.int64(PRIOR_SEED)}
    for name, x in inputs.items():
        out[name] = x
        m = x.astype(np.float64).mean(0).astype(np.float32)
        v = x.astype(np.float64).var(0, ddof=1).astype(np.float32)
        out[f'{name}/mean'], out[f'{name}/var'] = m, v
        for dt, tag in ((torch.float64, ''), (torch.float32, '_f32')):
            xt, mt, vt = (torch.from_numpy(t).to(dt) for t in (x, m, v))
            out[f'{name}/analytic_std{tag}'] = np.float64(ref.analytic_gaussian_rbf_mmd_sq(xt, True).item())
            out[f'{name}/analytic_raw{tag}'] = np.float64(ref.analytic_gaussian_rbf_mmd_sq(xt, False).item())
            out[f'{name}/custom_std{tag}'] = np.float64(ref.custom_gaussian_rbf_mmd_sq(xt, mt, vt, True).item())
            out[f'{name}/custom_raw{tag}'] = np.float64(ref.custom_gaussian_rbf_mmd_sq(xt, mt, vt, False).item())
            if x.shape[1] == 16:
                torch.manual_seed(PRIOR_SEED)
                # the reference's prior samples are f32 whatever x is, so its prior-prior term is an f32 pdist even
                # when x is f64: for the f64 record pdist widens its argument (same samples, f64 arithmetic)
                pdist = ref.F.pdist
                if dt == torch.float64:
                    ref.F.pdist = lambda t: pdist(t.double())
                try:
                    out[f'{name}/imq{tag}'] = np.float64(ref.gaussian_imq_mmd_sq(xt).item())
                finally:
                    ref.F.pdist = pdist
        if x.shape[1] == 16:
            lo = mmd_ref.imq_min_denominator(x, prior)
            print(f'{name}: min (s + d2 + offset) = {lo:.4f}')
            assert lo >= 1.0, (name, lo)
            out[f'{name}/imq_min_denominator'] = np.float64(lo)
    path = os.path.join(HERE, 'mmd.npz')
    np.savez_compressed(path, **out)
    for k in sorted(out):
        if np.ndim(out[k]) == 0:
            print(f'{k:28s} {float(out[k])!r}')
    print(f'{path}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
