"""-m gpu: the CRF transition-probability walk (csrc/crf_transitions.hip, crf_transitions_kernel) on the
device.  The table of tests/crf_transitions_cases.py on torch device tensors (fcd_crf_transition_probs_dev and
crf_transition_probs_batch_raw) against the float64 restatement (tests/crf_transitions_reference.py), the case whose LDS
passes 64 KiB (the launch that raises the kernel's limit), the edge cases, the argument errors and limits, the nullable logz,
host and device entry points bit for bit, torch tensors in and out without a synchronise, the pipeline scores -> probs ->
crf_beam_search -> crf_score under set_overlap(4) with no join in between.  Offsets past 2^31 elements and 2^32 bytes:
tests/test_gpu_far_offsets.py, test_far_walks."""
import numpy as np
import pytest

import crf_transitions_cases as TC
import crf_transitions_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.mark.parametrize("case", TC.CASES, ids=[c["name"] for c in TC.CASES])
def test_cases_on_device_tensors(fcd, case):
    TC.run_case(fcd, case, device="cuda")
    print("%s: err32 %.3g, device %.3g" % (case["name"], TC.build_case(case)["err32"], TC.OBSERVED[case["name"]]))


def test_lds_above_64_kib(fcd):
    TC.run_case(fcd, TC.BIG_LDS, device="cuda")
    print("%s: err32 %.3g, device %.3g" % (TC.BIG_LDS["name"], TC.build_case(TC.BIG_LDS)["err32"], TC.OBSERVED[TC.BIG_LDS["name"]]))


def test_edge_cases(fcd):
    TC.edge_cases(fcd, device="cuda")


def test_argument_errors_and_limits(fcd):
    TC.argument_errors(fcd, device="cuda")


def test_nullable_outputs(fcd):
    TC.nullable_outputs(fcd, device="cuda")


def test_host_and_device_entry_points_are_bitwise_equal(fcd):
    for name in ("s4_n5_t300_f16out", "s64_n5_t300_sd5", "s1024_n3_t130_f16_dest", "s12_n5_t7_dest_padded", "s3_n2_t300_tm"):
        c = TC.build_case([k for k in TC.CASES if k["name"] == name][0])
        host, dev = TC.call_abi(fcd, c), TC.call_abi(fcd, c, device="cuda")
        for b in range(c["B"]):
            TC.check_read(c, b, host[0][b], host[1][b], float(host[2][b]), host[3][b], ("host", name, b))
        for h, d, what in zip(host, dev, ("probs", "init", "logz", "status")):
            assert np.array_equal(h, d), (name, what)


def test_tensors_in_and_out_without_a_synchronise(fcd):
    """device tensors in, device tensors out, the searches read them on the same stream: nothing waits in between"""
    import torch
    rng = np.random.default_rng(31)
    x = TC.peaked_scores(rng, 4, 90, 64, 5)
    xd = torch.from_numpy(x).cuda().half()
    r = fcd.crf_transition_probs_batch_raw(xd, out_dtype="float16")
    for a in (r.probs, r.init, r.logz, r.status):
        assert a.is_cuda
    assert r.probs.dtype == torch.float16 and r.probs.shape == (4, 90, 64, 5)
    v = fcd.crf_viterbi_search_batch_raw(r.probs, r.init)   # reads probs and init on the device
    g = fcd.crf_greedy_search_batch_raw(r.probs.float(), r.init)
    v, g, rc = v.cpu(), g.cpu(), r.cpu()
    x16 = xd.cpu().float().numpy()
    for b in range(4):
        score, s0, rows, labels = TC.best_path64(x16[b])
        n = int(v.out_len[b])
        assert int(rc.status[b]) == 0 and v.labels[b, :n].tolist() == labels and v.path[b, :n].tolist() == rows
        assert g.labels[b, :int(g.out_len[b])].tolist() == labels
        ref = R.transitions64(x16[b])
        assert abs(rc.logz[b] - ref["logz"]) <= TC.logz_bound(ref["logz"])


def test_scores_to_beam_search_to_crf_score_under_overlap(fcd):
    """Four batches back to back under set_overlap(4): the transition probabilities on the handle's stream, the beam searches
    on internal streams behind it, the scores of their results ordered by the library -- no join in between"""
    import torch
    from fast_ctc_decode_amd import _native as nat
    rng = np.random.default_rng(12)
    xs = [torch.from_numpy(TC.peaked_scores(rng, 32, 120, 4, 5, gap=3.0)).cuda() for _ in range(4)]
    h = nat.default_handle(0)

    def pipeline():
        out = []
        for x in xs:
            r = fcd.crf_transition_probs_batch_raw(x, layout="source", out_dtype="float16", time_major_out=True)
            beam = fcd.crf_beam_search_batch_raw(r.probs, r.init, 8, 0.0)
            out.append((r, beam, beam.crf_score(r.probs, r.init)))
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        h.overlap_join()
        torch.cuda.synchronize()
        return [(r.cpu(), b.cpu(), s.cpu().numpy()) for r, b, s in out], out

    in_order, _ = pipeline()
    h.set_overlap(4)
    try:
        overlapped, keep = pipeline()
    finally:
        h.set_overlap(0)
    for (r0, b0, s0), (r1, b1, s1) in zip(in_order, overlapped):
        assert np.array_equal(r0.probs, r1.probs) and np.array_equal(r0.init, r1.init) and np.array_equal(r0.logz, r1.logz)
        assert (r0.status == 0).all() and (b0.status == 0).all()
        assert np.array_equal(b0.out_len, b1.out_len) and np.array_equal(s0, s1)
        for b in range(32):  # (entries beyond out_len are not written)
            assert np.array_equal(b0.labels[b, :int(b0.out_len[b])], b1.labels[b, :int(b0.out_len[b])]), b
        assert np.isfinite(s0).all() and (s0 <= 1e-3).all()
    x0 = xs[0].cpu().numpy()
    for b in (0, 17):
        ref = R.transitions64(x0[b])
        p = in_order[0][0].probs[b].astype(np.float64)
        assert np.abs(p - ref["probs"]).max() <= 2.0 ** -11 and abs(in_order[0][0].logz[b] - ref["logz"]) <= TC.logz_bound(ref["logz"])
