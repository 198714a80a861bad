"""-m gpu: the CRF Viterbi walk (csrc/crf_viterbi.hip, crf_viterbi_kernel) on the device.  The table of
tests/crf_viterbi_cases.py on torch device tensors (fcd_crf_viterbi_search_dev) against the restatement
(tests/crf_viterbi_reference.py) with the cross-checks against crf_align / crf_score / crf_greedy_search, one S = 4096,
N = 5 f16 case (80 KiB of LDS: the launch that raises the kernel's limit), the edge cases, the argument errors, the C ABI's
nullable pointers through _dev, several workspace groups, host and device entry points side by side, torch tensors in and
out without a synchronise, and the search -> crf_score pipeline under set_overlap(4) with no join in between."""
import numpy as np
import pytest

import crf_viterbi_cases as VC
import crf_viterbi_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


@pytest.mark.parametrize("case", VC.CASES, ids=[c[0] for c in VC.CASES])
def test_cases_on_device_tensors(fcd, case):
    VC.run_case(fcd, VC.build_case(case), device="cuda")


def test_lds_above_64_kib(fcd):
    c = VC.build_case(VC.BIG_LDS)
    VC.run_case(fcd, c, device="cuda")
    host = fcd.crf_viterbi_search_batch_raw(c["xin"], c["init"], c["lengths"], qual=True)
    for b in range(c["B"]):
        VC.check_read(host, b, c["refs"][b], ("host", c["name"], b))


def test_edge_cases(fcd):
    VC.edge_cases(fcd, device="cuda")


def test_tie_rules(fcd):
    VC.tie_rules(fcd, device="cuda")


def test_argument_errors_and_limits(fcd):
    VC.argument_errors(fcd, device="cuda")


def test_nullable_outputs(fcd):
    VC.nullable_outputs(fcd, device="cuda")


def test_workspace_cap_groups(fcd):
    VC.workspace_groups(fcd, device="cuda")


def test_host_and_device_entry_points_agree(fcd):
    for shape in ((64, 5, 300), (1024, 3, 65), (12, 5, 64)):
        c = VC.build_case([k for k in VC.CASES if k[1:4] == shape][0])
        kw = {"input_dtype": "bfloat16"} if c["dtype"] == "bf16" else {}
        host = fcd.crf_viterbi_search_batch_raw(c["xin"], c["init"], c["lengths"], qual=True, **kw)
        dev = VC.run_case(fcd, c, device="cuda", cross=False)
        for b in range(c["B"]):
            VC.check_read(host, b, c["refs"][b], ("host", c["name"], b))
            n = int(host.out_len[b])
            assert np.array_equal(dev.labels[b, :n], host.labels[b, :n]) and np.array_equal(dev.qual[b, :n], host.qual[b, :n])
        for k in ("out_len", "status", "logp"):
            assert np.array_equal(getattr(dev, k), getattr(host, k)), k


def test_tensors_in_and_out_without_a_synchronise(fcd):
    """device tensors in, device tensors out, the next call reads them on the same stream: nothing waits in between"""
    import torch
    rng = np.random.default_rng(31)
    x = np.stack([R.random_case(rng, 90, 64, 5)[0] for _ in range(4)])
    init = rng.random((4, 64)).astype(np.float32)
    xd, idv = torch.from_numpy(x).cuda(), torch.from_numpy(init).cuda()
    r = fcd.crf_viterbi_search_batch_raw(xd, idv, qual=True)
    for a in (r.labels, r.path, r.qual, r.out_len, r.status, r.logp):
        assert a.is_cuda
    al = r.crf_align(xd, idv)  # reads the search's labels and lengths on the device
    rc, al = r.cpu(), al.cpu()
    for b in range(4):
        VC.check_read(rc, b, R.viterbi(x[b], init[b]), ("no sync", b))
        n = int(rc.out_len[b])
        assert al.start[b, 0, :n].tolist() == rc.path[b, :n].astype(np.uint32).tolist()
        assert VC.same_logp(float(al.logp[b, 0]), float(rc.logp[b]))


def test_search_then_crf_score_under_overlap(fcd):
    """Four batches back to back under set_overlap(4): the beam searches go to internal streams, the Viterbi search and the
    scores of both results to the handle's stream, ordered by the library behind the searches in flight."""
    import torch
    from fast_ctc_decode_amd import _native as nat
    import crf_lattice_cases as CC
    rng = np.random.default_rng(12)
    xs = [torch.from_numpy(CC.posteriors(rng, 32, 120, 4, 5)).cuda() for _ in range(4)]
    init = torch.from_numpy(rng.random((32, 4)).astype(np.float32)).cuda()
    h = nat.default_handle(0)

    def pipeline():
        out = []
        for x in xs:
            beam = fcd.crf_beam_search_batch_raw(x, init, 8, 0.0)
            v = fcd.crf_viterbi_search_batch_raw(x, init)
            out.append((v, v.crf_score(x, init), beam.crf_align(x, init), beam))
        h.set_stream(torch.cuda.current_stream().cuda_stream)
        h.overlap_join()
        torch.cuda.synchronize()
        return [(v.cpu(), s.cpu().numpy(), a.cpu()) for v, s, a, _ in out], out

    in_order, _ = pipeline()
    h.set_overlap(4)
    try:
        overlapped, keep = pipeline()
    finally:
        h.set_overlap(0)
    x0, i0 = xs[0].cpu().numpy(), init.cpu().numpy()
    for (v0, s0, a0), (v1, s1, a1) in zip(in_order, overlapped):
        assert np.array_equal(v0.labels, v1.labels) and np.array_equal(v0.out_len, v1.out_len) and np.array_equal(v0.logp, v1.logp)
        assert np.array_equal(s0, s1) and np.isfinite(s0).all() and (s0[:, 0] >= v0.logp - CC.tolerance(120)).all()
        # the Viterbi path's probability is no less than the best alignment of the beam search's labelling
        assert (v1.logp >= a1.logp[:, 0] - 2.0 ** -40 * np.abs(a1.logp[:, 0])).all()
    for b in (0, 17):
        VC.check_read(_with_qual(fcd, xs[0], init, overlapped[0][0]), b, R.viterbi(x0[b], i0[b]), ("overlap", b))


def _with_qual(fcd, x, init, r):
    """(the pipeline ran without qualities: the same search with them, for check_read)"""
    q = fcd.crf_viterbi_search_batch_raw(x, init, qual=True).cpu()
    assert np.array_equal(q.labels[:, :1], r.labels[:, :1]) and np.array_equal(q.out_len, r.out_len) and np.array_equal(q.logp, r.logp)
    return q
