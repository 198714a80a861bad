"""TEST INFRASTRUCTURE: what fcd_crf_viterbi_search_* computes (include/fcd.h), restated in numpy straight from the
definition -- the specification the kernel (csrc/crf_viterbi.hip, crf_viterbi_kernel) is held to -- and a float64 enumeration of
every label sequence of a tiny case.

sigma_0 = the first maximum of the init row; v_{-1}[sigma_0] = 1.  For every state s' with j = s' mod nb, q = S / nb,
s_i = s' div nb + i q:
    v_t[s'] = max( v_{t-1}[s'] p_t[s'][0] ,  max_i v_{t-1}[s_i] p_t[s_i][j+1] )
the stay candidate kept unless an advance is strictly greater, the lowest i among equal advances, the end state the first
maximum of the last row.  A value is an f32 mantissa in [0.5, 1) (np.float32, so that a product rounds as the kernel's
does) with a Python-int exponent -- "f32 with an unbounded exponent", crf_lattice_reference's form; each candidate is ONE
f32 product.  Nothing is dropped unless asked for (drop): the kernel may drop a cell below 2^-160 of its row's maximum."""
import itertools
import math

import numpy as np

from crf_lattice_reference import ZERO_E, _gt

ST_OK, ST_INCOMPARABLE, ST_BAD_STATE = 0, 2, 4


def first_max(row):
    """index of the first maximum, or None for an empty row or one that holds a NaN (greedy's rule)"""
    row = np.asarray(row, np.float32)
    if row.size == 0 or np.isnan(row).any():
        return None
    best = 0
    for i, v in enumerate(row):
        if v > row[best]:
            best = i
    return best


def _fail(status):
    return dict(status=status, labels=[], path=[], qual=[], logp=math.nan)


def viterbi(p, init, drop=None):
    """p: (T, S, N) float32, init: (n_init,) -> dict(status, labels, path, qual (np.float32), logp).  drop = 2^-k: cells
    below that fraction of their row's maximum become 0 -- what the contract lets the kernel do; a case whose result
    differs with drop=2^-160 relies on such cells."""
    p = np.asarray(p)
    assert p.dtype == np.float32 and p.ndim == 3
    T, S, N = p.shape
    nb = N - 1
    assert nb >= 1 and S % nb == 0
    q = S // nb
    s0 = first_max(init)
    if s0 is None:
        return _fail(ST_BAD_STATE)
    if T == 0:
        return dict(status=ST_OK, labels=[], path=[], qual=[], logp=0.0)
    if s0 >= S:
        return _fail(ST_BAD_STATE)
    if np.isnan(p).any():
        return _fail(ST_INCOMPARABLE)
    vm = np.zeros(S, np.float32)
    ve = np.full(S, ZERO_E, np.int64)
    vm[s0], ve[s0] = 0.5, 1
    bp = np.zeros((T, S), np.uint8)
    dest = np.arange(S)
    for t in range(T):
        pm, pe = np.frexp(p[t])                      # (S, N) mantissas (float32) and exponents
        prod = vm[:, None] * pm                      # f32 x f32: one rounding per candidate
        assert prod.dtype == np.float32
        fm, fe = np.frexp(prod)
        ce = np.where(prod > 0, ve[:, None] + pe.astype(np.int64) + fe.astype(np.int64), ZERO_E)
        cm = np.where(prod > 0, fm, np.float32(0)).astype(np.float32)
        bm, be = cm[:, 0].copy(), ce[:, 0].copy()    # the stay candidate
        for i in range(nb):
            src = dest // nb + i * q
            am, ae = cm[src, dest % nb + 1], ce[src, dest % nb + 1]
            up = (ae > be) | ((ae == be) & (am > bm))  # strictly greater only
            bm, be = np.where(up, am, bm), np.where(up, ae, be)
            bp[t, up] = i + 1
        vm, ve = bm.astype(np.float32), be
        if drop is not None and (vm > 0).any():
            cut = int(round(math.log2(drop)))
            assert 2.0 ** cut == drop
            top = max(range(S), key=lambda d: (ve[d], vm[d]) if vm[d] > 0 else (ZERO_E, 0))
            low = (vm > 0) & ((ve < ve[top] + cut) | ((ve == ve[top] + cut) & (vm < vm[top])))
            vm, ve = np.where(low, np.float32(0), vm), np.where(low, ZERO_E, ve)
    end = 0
    for d in range(S):
        if _gt(vm[d], ve[d], vm[end], ve[end]):
            end = d
    logp = (math.log(float(vm[end])) + int(ve[end]) * math.log(2.0)) if vm[end] > 0 else -math.inf
    labels, path, qual = [], [], []
    d = end
    for t in range(T - 1, -1, -1):
        b = int(bp[t, d])
        if b:
            j = d % nb
            s = d // nb + (b - 1) * q
            labels.append(j + 1)
            path.append(t)
            qual.append(np.float32(p[t, s, j + 1]))
            d = s
    return dict(status=ST_OK, labels=labels[::-1], path=path[::-1], qual=qual[::-1], logp=logp)


def greedy(p, init):
    """search::crf_greedy_search (src/search.rs:385-423) -> (labels, path, qual, ln of the product along its path)"""
    p = np.asarray(p, np.float32)
    T, S, N = p.shape
    nb = N - 1
    s = first_max(init)
    labels, path, qual, logw = [], [], [], 0.0
    for t in range(T):
        row = p[t, s]
        a = first_max(row)
        logw += math.log(float(row[a])) if row[a] > 0 else -math.inf
        if a > 0:
            labels.append(a)
            path.append(t)
            qual.append(np.float32(row[a]))
            s = (s * nb) % S + (a - 1)
    return labels, path, qual, logw


def enumerate_paths(p, init):
    """Every sequence of T symbols (0 = stay, j = emit label j) with its float64 probability under the searches' transition
    (src/search.rs:97,414), best first: [(probability, labels, path)]"""
    p = np.asarray(p, np.float32).astype(np.float64)
    T, S, N = p.shape
    nb = N - 1
    s0 = first_max(init)
    out = []
    for seq in itertools.product(range(N), repeat=T):
        w, s = 1.0, s0
        for t, a in enumerate(seq):
            w *= p[t, s, a]
            if a:
                s = (s * nb) % S + (a - 1)
        out.append((w, [a for a in seq if a], [t for t, a in enumerate(seq) if a]))
    out.sort(key=lambda x: -x[0])
    return out


def random_case(rng, T, S, N, alpha=0.5, floor=2.0 ** -20):
    """Dirichlet(alpha) rows floored at `floor`, and an init row"""
    p = rng.dirichlet([alpha] * N, size=(T, S)).astype(np.float32)
    p = np.maximum(p, np.float32(floor))
    return p, rng.random(S).astype(np.float32)
