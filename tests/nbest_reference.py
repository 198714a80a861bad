"""TEST INFRASTRUCTURE: the n best hypotheses of search::beam_search / search::crf_beam_search.

The oracle returns beam[0] only, as the reference does (src/search.rs:165,300).  This is a restatement of both searches
(src/search.rs:159-301, :38-157) that returns the WHOLE final beam -- as it stands after the last row's truncation and
division by the top probability -- built on tests/naive_reference.py's SuffixTree, Point1, f32 and f32_div.  Equal
probabilities are ranked as the reference's sort_unstable_by ranks them: up to 20 candidates (and always, with
stable=True) the stable order of the node-ordered list; above 20 the oracle's restatement of Rust 1.78's quicksort
(oracle.pdqsort_desc, the one the kernels replay).

Each result is (status, hypotheses); a hypothesis is (labels, path, score): alphabet indices (1 .. N-1) in sequence
order, the creation time of each node, and SearchPoint::probability() of the entry in f32.  Statuses are FCD_ST_*."""
import numpy as np

from naive_reference import ROOT_NODE, Point1, SuffixTree, f32, f32_div

OK, RAN_OUT_OF_BEAM, INCOMPARABLE, BAD_STATE = 0, 1, 2, 4


def _rank(merged, stable):
    """sort_unstable_by(probability desc) of the node-ordered list, or None if it compares a NaN (:122,262)"""
    probs = [x.probability() for x in merged]
    if len(merged) >= 2 and any(p != p for p in probs):
        return None
    if stable or len(merged) <= 20:
        return sorted(merged, key=lambda x: -x.probability())
    from oracle import oracle
    _, nodes = oracle.pdqsort_desc(np.array(probs, np.float32), np.array([x.node for x in merged], np.int32))
    by_node = {x.node: x for x in merged}
    return [by_node[int(n)] for n in nodes]


def _merge(next_beam):
    merged = []
    for item in sorted(next_beam, key=lambda x: x.node):  # stable sort by node, then fold (:245-260)
        if merged and merged[-1].node == item.node:
            merged[-1].label_prob = f32(merged[-1].label_prob + item.label_prob)
            merged[-1].gap_prob = f32(merged[-1].gap_prob + item.gap_prob)
        else:
            merged.append(item)
    return merged


def _prune(next_beam, beam_size, stable):
    ranked = _rank(_merge(next_beam), stable)
    if ranked is None:
        return INCOMPARABLE, None
    beam = ranked[:beam_size]
    if not beam:
        return RAN_OUT_OF_BEAM, None
    top = beam[0].probability()
    for x in beam:
        x.label_prob = f32_div(x.label_prob, top)
        x.gap_prob = f32_div(x.gap_prob, top)
    return OK, beam


def _hypotheses(tree, beam, n_best):
    out = []
    for p in beam[:n_best]:
        labels, path = [], []
        for label, time in tree.iter_from(p.node):
            labels.append(label + 1)
            path.append(time)
        out.append((labels[::-1], path[::-1], p.probability()))
    return out


def beam_search(x, beam_size, thr, collapse_repeats=True, n_best=None, stable=False):
    """x: (T, N) float32 -> (status, hypotheses)"""
    rows = np.asarray(x, np.float32).tolist()
    n_best = beam_size if n_best is None else n_best
    thr = f32(thr)
    alphabet_size = np.asarray(x).shape[1] - 1
    tree = SuffixTree(alphabet_size)
    beam = [Point1(ROOT_NODE, 0, 0.0, 1.0)]
    for idx, pr in enumerate(rows):
        next_beam = []
        for b in beam:
            tip_label = tree.label(b.node)
            if pr[0] > thr:
                next_beam.append(Point1(b.node, 0, 0.0, f32(f32(b.label_prob + b.gap_prob) * pr[0])))
            for label in range(alphabet_size):
                pr_b = pr[label + 1]
                if pr_b < thr:
                    continue
                if collapse_repeats and label == tip_label:
                    next_beam.append(Point1(b.node, 0, f32(b.label_prob * pr_b), 0.0))
                    new_node = tree.get_child(b.node, label)
                    if new_node is None and b.gap_prob > 0.0:
                        new_node = tree.add_node(b.node, label, idx)
                    if new_node is not None:
                        next_beam.append(Point1(new_node, 0, f32(b.gap_prob * pr_b), 0.0))
                else:
                    new_node = tree.get_child(b.node, label)
                    if new_node is None:
                        new_node = tree.add_node(b.node, label, idx)
                    next_beam.append(Point1(new_node, 0, f32(f32(b.label_prob + b.gap_prob) * pr_b), 0.0))
        st, beam = _prune(next_beam, beam_size, stable)
        if st != OK:
            return st, []
    return OK, _hypotheses(tree, beam, n_best)


def crf_beam_search(x, init_state, beam_size, thr, n_best=None, stable=False):
    """x: (T, S, N) float32, init_state: (n_init,) float32 -> (status, hypotheses); labels in sequence order (the
    reference's character reversal, :146-156, only concerns the strings)"""
    probs = np.asarray(x, np.float32).tolist()
    init = np.asarray(init_state, np.float32).tolist()
    n_best = beam_size if n_best is None else n_best
    thr = f32(thr)
    T, n_state, N = np.asarray(x).shape
    n_base = N - 1
    tree = SuffixTree(n_base)
    best = 0
    for i, v in enumerate(init):  # argmax / max: the first maximum; NaN: the reference panics
        if v != v:
            return BAD_STATE, []
        if v > init[best]:
            best = i
    beam = [Point1(ROOT_NODE, best, init[best], init[0])]
    for idx in range(T):
        next_beam = []
        for b in beam:
            if b.state >= n_state:  # ndarray index out of bounds: the reference panics
                return BAD_STATE, []
            pr = probs[idx][b.state]
            if pr[0] > thr:
                next_beam.append(Point1(b.node, b.state, 0.0, f32(f32(b.label_prob + b.gap_prob) * pr[0])))
            for label in range(n_base):
                pr_b = pr[label + 1]
                if pr_b < thr:
                    continue
                child = tree.get_child(b.node, label)
                if child is None:
                    child = tree.add_node(b.node, label, idx)
                next_beam.append(Point1(child, (b.state * n_base) % n_state + label,
                                        f32(f32(b.label_prob + b.gap_prob) * pr_b), 0.0))
        st, beam = _prune(next_beam, beam_size, stable)
        if st != OK:
            return st, []
    return OK, _hypotheses(tree, beam, n_best)
