"""The duplex searches on ragged, 16-bit and strided batches, on the GPU: lengths_1 / lengths_2, float16 / bfloat16 / mixed
element types and arbitrary strides through env_width_kernel, ln_convert_kernel, duplex_kernel (csrc/duplex.hip) and
duplex_slots_kernel (csrc/duplex_slots.hip), device tensors and the host staging of csrc/capi.hip.  Every pair of every
launch is compared with the correctly rounded oracle on the TRUNCATED pair (tests/duplex_ragged_cases.py: the cases, the
poison beyond every pair's own rows, the runner); tests/test_duplex_ragged_emu.py asserts from the oracle alone that
no launch here can pass vacuously, and runs a selection on the emulated kernels."""
import numpy as np
import pytest

import duplex_ragged_cases as RC

pytestmark = pytest.mark.gpu

LSE, MAX = RC.LSE, RC.MAX
MODE_IDS = ["logsumexp", "max"]
KERNEL_IDS = ["auto", "any-shape", "slot-resident"]
MIXED = (("f16", "f16"), ("bf16", "bf16"), ("f16", "f32"), ("f32", "bf16"), ("bf16", "f16"))


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    return torch.device("cuda:0")


@pytest.mark.parametrize("flavour", RC.FLAVOURS, ids=["band-per-pair", "band-for-the-caps", "default-envelope"])
@pytest.mark.parametrize("which", [0, 1, 2], ids=KERNEL_IDS)
@pytest.mark.parametrize("mode", RC.MODES, ids=MODE_IDS)
def test_ragged_every_kernel(fcd, dev, mode, which, flavour):
    """Device tensors, plain and CRF, each kernel forced.  With the slot-resident kernel forced the band for the caps must
    still be accepted: its 2^40-wide rows lie beyond l1 and belong to no pair.  The per-pair band runs on numpy inputs
    too (the staging of duplex_host): device and host results equal each other as well as the oracle."""
    with RC.forced_kernel(which):
        plain = RC.run(fcd, "plain", flavour, mode, device=dev)
        crf = RC.run(fcd, "crf", flavour, mode, device=dev)
        if flavour == 2:
            RC.run(fcd, "plain", flavour, mode, collapse=False, device=dev)
        if flavour == 1:
            RC.same(RC.run(fcd, "plain", flavour, mode), plain)
            RC.same(RC.run(fcd, "crf", flavour, mode), crf)


@pytest.mark.parametrize("which", [1, 2], ids=KERNEL_IDS[1:])
def test_ragged_tie_counters(fcd, dev, which):
    """fcd_result.ambiguous of the ragged launch == the oracle's counters of the truncated pair, pair by pair (the
    failing pair 4, whose search stops on its envelope, has counted by then; a pair without rows counts nothing)"""
    with RC.forced_kernel(which):
        r = RC.run(fcd, "plain", 1, MAX, device=dev, count_ambiguous=True)
        assert np.asarray(r.ambiguous).any()
        RC.same(RC.run(fcd, "plain", 1, MAX, count_ambiguous=True), r)


@pytest.mark.parametrize("which", [0, 1, 2], ids=KERNEL_IDS)
def test_one_wide_pair_and_chunks(fcd, dev, which):
    """Pair 5 gets the full matrix, (0, l2) on every row: width 51 decides the ring size and the staging of the whole
    batch.  Every pair still equals the oracle, the seven narrow pairs equal their results from the launch without the
    wide pair, and under a workspace limit (RC.chunk_limit: three pairs per launch) nothing changes -- the search kernels
    index their slabs by the pair's place in the chunk, their inputs and outputs by the pair."""
    case = RC.plain_case()
    narrow = [i for i in range(case.B) if i != RC.WIDE_PAIR]
    with RC.forced_kernel(which) as h:
        whole = {}
        for mode in RC.MODES:
            base = RC.run(fcd, "plain", 1, mode, device=dev, count_ambiguous=True)
            whole[mode] = RC.run(fcd, "plain", 1, mode, device=dev, wide=RC.WIDE_PAIR, count_ambiguous=True)
            RC.same(whole[mode], base, narrow)
        h.release_workspace()  # (the arena the unchunked launches left would hold a slab per pair)
        h.set_workspace_limit(RC.chunk_limit(case, which, int(case.l2[RC.WIDE_PAIR])))
        try:
            for mode in RC.MODES:
                RC.same(RC.run(fcd, "plain", 1, mode, device=dev, wide=RC.WIDE_PAIR, count_ambiguous=True), whole[mode])
            RC.same(RC.run(fcd, "plain", 1, MAX, wide=RC.WIDE_PAIR, count_ambiguous=True), whole[MAX])  # host staging
        finally:
            h.set_workspace_limit(0)


@pytest.mark.parametrize("mode", RC.MODES, ids=MODE_IDS)
def test_rows_beyond_l1_do_not_size_the_rings(fcd, dev, mode):
    """RC.tall_case: T2cap = 600, more rows than the slot-resident kernel's rings can hold.  Forced, that kernel takes the
    launches whose 2^40-wide rows lie beyond l1 -- env_width_kernel must not count them -- and refuses the one in which
    pair 0 really has 600-row windows (FCD_E_UNSUPPORTED: the threshold is crossed at this size); AUTO decodes that one
    with the any-shape kernel.  Every accepted launch equals the oracle."""
    nat = fcd.api.nat
    with RC.forced_kernel(2):
        RC.run(fcd, "tall", 1, mode, device=dev)
        RC.run(fcd, "tall", 2, mode, device=dev)
        RC.run(fcd, "tall", 1, mode)
        with pytest.raises(nat.NativeError) as e:
            RC.run(fcd, "tall", 1, mode, wide=0, device=dev)
        assert e.value.code == nat.E_UNSUPPORTED
    RC.run(fcd, "tall", 1, mode, wide=0, device=dev)


@pytest.mark.parametrize("dtypes", MIXED, ids=["-".join(d) for d in MIXED])
@pytest.mark.parametrize("mode", RC.MODES, ids=MODE_IDS)
def test_element_types(fcd, dev, mode, dtypes):
    """Each read converts with its OWN element type; an exact 1.0, an exact 0.0 and a float16 subnormal sit in live rows
    of read 2.  The oracle runs on the exact float32 upcast of what the kernel is given."""
    RC.run(fcd, "plain", 1, mode, dtypes=dtypes, device=dev)
    if dtypes in (("f16", "f16"), ("f16", "f32")):
        RC.run(fcd, "crf", 1, mode, dtypes=dtypes, device=dev)
        RC.run(fcd, "plain", 1, mode, dtypes=dtypes)   # numpy float16
        RC.run(fcd, "crf", 1, mode, dtypes=dtypes)


@pytest.mark.parametrize("layouts", [("time", "batch"), ("batch", "time"), ("time", "time"), ("view", "view")],
                         ids=lambda l: "-".join(l))
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("host", [False, True], ids=["device", "numpy"])
def test_strides(fcd, dev, host, dtype, layouts):
    """Time-major storage -- a (T, B, N) / (T, B, S, N) array handed over as its transpose -- for read 1 only, read 2
    only and both; a column and row view big[:, ::2, 1:6] of a (B, 2 * Tcap, 8) array of NaNs for both reads.  Ragged,
    both modes (the per-pair band under one, the band for the caps under the other)."""
    d = None if host else dev
    for mode, flavour in ((LSE, 1), (MAX, 2)):
        RC.run(fcd, "plain", flavour, mode, dtypes=(dtype, dtype), layouts=layouts, device=d)
        if "view" not in layouts:
            RC.run(fcd, "crf", flavour, mode, dtypes=(dtype, dtype), layouts=layouts, device=d)


@pytest.mark.parametrize("host", [False, True], ids=["device", "numpy"])
@pytest.mark.parametrize("mode", RC.MODES, ids=MODE_IDS)
def test_estimator_in_the_loop(fcd, dev, mode, host):
    """estimate_envelope_batch on the ragged case, poison in place, feeds the search with the same lengths: the envelope
    rows of every pair are tests/envelope_model.py's on the truncated pair, the result the oracle's inside them."""
    RC.estimator_loop(fcd, mode, None if host else dev)
