"""CPU-side check of the duplex searches on ragged, float16 and strided batches (tests/duplex_ragged_cases.py) on
tests/hipemu's lockstep emulation: numpy inputs through the host entries, every pair against the oracle on the truncated
pair.  The first two tests establish, from the oracle alone, that no launch of this file or of its -m gpu twin
(tests/test_gpu_duplex_ragged.py) can pass vacuously."""
import numpy as np
import pytest

import duplex_ragged_cases as RC
from emu_util import emulated_kernels

LSE, MAX = RC.LSE, RC.MAX
MIXED = (("f16", "f16"), ("bf16", "bf16"), ("f16", "f32"), ("f32", "bf16"), ("bf16", "f16"))


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


def test_every_launch_has_pairs_that_decode_and_pairs_that_fail():
    for mode in RC.MODES:
        for flavour in RC.FLAVOURS:
            RC.check_conditions("plain", flavour, mode)
            RC.check_conditions("crf", flavour, mode)
        RC.check_conditions("plain", 2, mode, collapse=False)
        RC.check_conditions("plain", 1, mode, wide=RC.WIDE_PAIR)
        for dtypes in MIXED:
            RC.check_conditions("plain", 1, mode, dtypes=dtypes)
        for dtypes in MIXED[0], MIXED[2]:
            RC.check_conditions("crf", 1, mode, dtypes=dtypes)
    # the cases are what they are named after
    p, c = RC.plain_case(), RC.crf_case()
    for case in (p, c):
        for lens, cap in ((case.l1, case.T1), (case.l2, case.T2)):
            assert {0, 1, cap - 1, cap} <= set(int(v) for v in lens) and sum(1 < v < cap - 1 for v in lens) >= 2
    S = c.clean1.shape[2]
    assert c.init1.shape == c.init2.shape == (c.B, S + 1)
    assert int(np.argmax(c.init1[2])) == S and c.l1[2] > 0 and c.l2[2] > 0   # a start state out of range, nothing else wrong
    assert (c.init1[1] == c.init1[1, 0]).all() and (c.init2[1] == c.init2[1, 0]).all()
    assert RC.decoded(RC.truth("crf", 1, LSE)[1][0]) and not RC.decoded(RC.truth("crf", 1, LSE)[2][0])
    _, q2, _, up2 = p.reads(("f16", "f16"))
    assert up2[0, 20, 2] == 1.0 and up2[5, 30, 0] == 0.0 and 0 < up2[6, 10, 3] < 2.0 ** -14  # 1, 0 and a subnormal, in live rows
    assert p.l2[0] > 20 and p.l2[5] > 30 and p.l2[6] > 10
    assert any(amb != (0, 0) for _, amb in RC.truth("plain", 1, MAX))  # the tie counters compared are not all zero
    # the poison: NaN rows beyond the lengths, both kinds of envelope row beyond l1
    q1, q2, _, _ = p.reads()
    env = RC.envelopes(p, 2)
    for i in range(p.B):
        assert np.isnan(q1[i, p.l1[i]:]).all() and np.isnan(q2[i, p.l2[i]:]).all()
        assert not np.isnan(q1[i, :p.l1[i]]).any() and not np.isnan(q2[i, :p.l2[i]]).any()
        rows = set(tuple(int(v) for v in row) for row in env[i, p.l1[i]:])
        assert rows <= set(RC.POISON_ROWS) and (p.T1 - p.l1[i] < 2 or rows == set(RC.POISON_ROWS))


@pytest.mark.parametrize("mode", RC.MODES, ids=["logsumexp", "max"])
def test_a_kernel_that_ignored_lengths_2_would_be_caught(mode):
    for name in ("plain", "crf"):
        RC.check_lengths_matter(name, 2, mode)   # bounds clamped to the pair's own T2 (and fatal on row 0)


@pytest.mark.parametrize("mode", RC.MODES, ids=["logsumexp", "max"])
@pytest.mark.parametrize("which", [1, 2], ids=["any-shape", "slot-resident"])
def test_ragged(fcd, which, mode):
    """flavour 2 under the slot-resident kernel: the 2^40-wide rows belong to no pair, the launch must be accepted"""
    with RC.forced_kernel(which):
        for flavour in (1, 2):
            RC.run(fcd, "plain", flavour, mode, count_ambiguous=(flavour == 1))
            RC.run(fcd, "crf", flavour, mode)
        RC.run(fcd, "plain", 2, mode, collapse=False)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["auto", "any-shape", "slot-resident"])
def test_one_wide_pair_and_chunks(fcd, which):
    """pair 5's full-matrix envelope sizes the rings of the whole batch; under a workspace limit the same launch runs three
    pairs at a time and every kernel indexes its slabs by the pair's place in the chunk"""
    case = RC.plain_case()
    narrow = [i for i in range(case.B) if i != RC.WIDE_PAIR]
    with RC.forced_kernel(which) as h:
        whole = {}
        for mode in RC.MODES:
            base = RC.run(fcd, "plain", 1, mode, count_ambiguous=True)
            whole[mode] = RC.run(fcd, "plain", 1, mode, wide=RC.WIDE_PAIR, count_ambiguous=True)
            RC.same(whole[mode], base, narrow)
        h.release_workspace()  # (the arena the unchunked launches left would hold a slab per pair)
        h.set_workspace_limit(RC.chunk_limit(case, which, int(case.l2[RC.WIDE_PAIR])))
        try:
            for mode in RC.MODES:
                RC.same(RC.run(fcd, "plain", 1, mode, wide=RC.WIDE_PAIR, count_ambiguous=True), whole[mode])
        finally:
            h.set_workspace_limit(0)


@pytest.mark.parametrize("mode", RC.MODES, ids=["logsumexp", "max"])
def test_float16_host_arrays(fcd, mode):
    for dtypes in (("f16", "f16"), ("f16", "f32")):
        RC.run(fcd, "plain", 1, mode, dtypes=dtypes)
    RC.run(fcd, "crf", 1, mode, dtypes=("f16", "f32"))


def test_time_major_and_views(fcd):
    RC.run(fcd, "plain", 1, LSE, dtypes=("f16", "f32"), layouts=("time", "batch"))
    RC.run(fcd, "crf", 2, MAX, layouts=("batch", "time"))
    RC.run(fcd, "plain", 2, MAX, layouts=("view", "view"))


def test_rows_beyond_l1_do_not_size_the_rings(fcd):
    """(tall_case) forced, the slot-resident kernel takes the launch whose 2^40-wide rows lie beyond l1 and refuses the
    one in which pair 0 really has 600-row windows; AUTO decodes that one with the any-shape kernel"""
    nat = fcd.api.nat
    for mode in RC.MODES:
        RC.check_conditions("tall", 1, mode)
        RC.check_conditions("tall", 2, mode)
        RC.check_conditions("tall", 1, mode, wide=0)
        with RC.forced_kernel(2):
            RC.run(fcd, "tall", 1, mode)
            RC.run(fcd, "tall", 2, mode)
            with pytest.raises(nat.NativeError) as e:
                RC.run(fcd, "tall", 1, mode, wide=0)
            assert e.value.code == nat.E_UNSUPPORTED
        RC.run(fcd, "tall", 1, mode, wide=0)


def test_estimator_in_the_loop(fcd):
    RC.estimator_loop(fcd, LSE)
