"""Which calls the labelling-lattice layer of fast_ctc_decode_amd/api.py refuses, and with which exception: a table recorded
before the ten *_batch_raw bodies and the twenty result methods were folded into one each, on numpy inputs over tests/hipemu's
emulation of the kernels.  The asymmetries between BatchResult and NBestResult are part of the table: they are behaviour."""
import numpy as np
import pytest

from emu_util import emulated_kernels

KINDS = ("score", "align", "posterior", "edits", "occupancy")
CALLS = [(m, k) for m in ("ctc", "crf") for k in KINDS]
B, T, N, S, STRIDE = 2, 8, 5, 4, 6


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    with emulated_kernels():
        yield m


def posteriors(model, b=B, t=T, n=N):
    rng = np.random.default_rng(3)
    x = rng.random((b, t, S, n) if model == "crf" else (b, t, n)).astype(np.float32) + 0.05
    return x / x.sum(tuple(range(2, x.ndim)), keepdims=True)


def arguments(model, n_hyp=1):
    """a call that is in order: (positional arguments, keyword arguments)"""
    shape = (B, STRIDE) if n_hyp == 1 else (B, n_hyp, STRIDE)
    labels = np.full(shape, 2, np.uint8)
    labels[..., 1::2] = 3
    args = dict(x=posteriors(model), init=np.ones((B, S), np.float32), labels=labels,
                ylen=np.full(shape[:-1], 3, np.uint32))
    return args, dict(lengths=np.array([T, T - 3], np.int64))


def call(fcd, model, kind, n_hyp=1, **change):
    a, kw = arguments(model, n_hyp)
    for k in list(change):
        if k in a:
            a[k] = change.pop(k)
    kw.update(change)
    head = (a["x"], a["init"]) if model == "crf" else (a["x"],)
    return getattr(fcd, "%s_%s_batch_raw" % (model, kind))(*head, a["labels"], a["ylen"], **kw)


PATHS = np.tile(np.arange(STRIDE, dtype=np.uint32), (B, 1))

# name -> (changes to a call that is in order, the exception)
BAD_CALLS = {
    "negative band": (dict(band=-1, paths=PATHS), ValueError),
    "float band": (dict(band=2.0, paths=PATHS), TypeError),
    "bool band": (dict(band=True, paths=PATHS), TypeError),
    "band without paths": (dict(band=2), ValueError),
    "paths of the wrong shape": (dict(band=2, paths=PATHS[:, :STRIDE - 1]), ValueError),
    "labels of another leading dimension": (dict(labels=np.ones((B + 1, STRIDE), np.uint8)), ValueError),
    "label_lengths of the wrong count": (dict(ylen=np.ones(B + 1, np.uint32)), ValueError),
    "n_valid of the wrong shape": (dict(n_valid=np.ones(B + 1, np.uint32)), ValueError),
}


@pytest.mark.parametrize("name", sorted(BAD_CALLS))
@pytest.mark.parametrize("model,kind", CALLS, ids=["%s_%s" % c for c in CALLS])
def test_batch_call_refuses(fcd, model, kind, name):
    change, exc = BAD_CALLS[name]
    with pytest.raises(exc):
        call(fcd, model, kind, **change)


@pytest.mark.parametrize("model,kind", CALLS, ids=["%s_%s" % c for c in CALLS])
def test_batch_call_refuses_posteriors_of_the_wrong_rank(fcd, model, kind):
    other = "ctc" if model == "crf" else "crf"
    with pytest.raises(TypeError):
        call(fcd, model, kind, x=posteriors(other))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("init", [np.ones((B + 1, S), np.float32), np.ones(S, np.float32), np.ones((B, 0), np.float32)],
                         ids=["rows", "rank", "empty"])
def test_crf_call_refuses_init_states_of_the_wrong_shape(fcd, kind, init):
    with pytest.raises(ValueError):
        call(fcd, "crf", kind, init=init)


def occupancy_buffer(model, shape=None, dtype=np.float32):
    return np.zeros(shape or ((B, T, S, N) if model == "crf" else (B, T, N)), dtype)


def _read_only(model):
    out = occupancy_buffer(model)
    out.flags.writeable = False
    return out


BAD_OCCUPANCY = {
    "accumulate without out": (lambda m: dict(accumulate=True), ValueError),
    "out with time_major_out": (lambda m: dict(out=occupancy_buffer(m), time_major_out=True), ValueError),
    "out of the wrong dtype": (lambda m: dict(out=occupancy_buffer(m, dtype=np.float64)), TypeError),
    "out of the wrong shape": (lambda m: dict(out=occupancy_buffer(m, (B, T - 1, S, N) if m == "crf" else (B, T - 1, N))),
                               ValueError),
    "out of the wrong rank": (lambda m: dict(out=occupancy_buffer(m, (B * T * N,))), ValueError),
    "out with rows that are not dense": (  # (the row: S * N floats under the CRF model, N under plain CTC)
        lambda m: dict(out=occupancy_buffer(m, (B, T, S, N + 1))[..., :N] if m == "crf" else
                       occupancy_buffer(m, (B, T, 2 * N))[..., ::2]), ValueError),
    "out that is read-only": (lambda m: dict(out=_read_only(m)), TypeError),
    "out that is no array": (lambda m: dict(out=[0.0] * (B * T * N)), TypeError),
}


@pytest.mark.parametrize("name", sorted(BAD_OCCUPANCY))
@pytest.mark.parametrize("model", ("ctc", "crf"))
def test_occupancy_refuses(fcd, model, name):
    change, exc = BAD_OCCUPANCY[name]
    with pytest.raises(exc):
        call(fcd, model, "occupancy", **change(model))


def test_occupancy_refuses_before_it_reads_the_inputs(fcd):
    """both ValueErrors about out come before the inputs are looked at: the labels here are of no use either"""
    for model in ("ctc", "crf"):
        with pytest.raises(ValueError, match="accumulate=True needs"):
            call(fcd, model, "occupancy", labels=np.ones((B + 1, STRIDE), np.uint8), accumulate=True)
        with pytest.raises(ValueError, match="pass either out or time_major_out"):
            call(fcd, model, "occupancy", labels=np.ones((B + 1, STRIDE), np.uint8), out=occupancy_buffer(model),
                 time_major_out=True)
        with pytest.raises(ValueError, match="band must be at least 0"):
            call(fcd, model, "occupancy", band=-1, accumulate=True)


# ---- the results' methods -------------------------------------------------------------------
@pytest.fixture(scope="module")
def results(fcd):
    from fast_ctc_decode_amd import api
    x, xc, init = posteriors("ctc"), posteriors("crf"), np.ones((B, S), np.float32)
    plain = fcd.beam_search_batch_raw(x, 5, 0.0)
    crf_search = fcd.crf_beam_search_batch_raw(xc, init, 5, 0.0)
    # (the CRF beam search returns a BatchResult; the sessions and the CRF Viterbi search a _CrfBatchResult of such arrays)
    crf = api._CrfBatchResult(crf_search.labels, crf_search.path, crf_search.out_len, crf_search.status)
    assert type(plain) is api.BatchResult and type(crf_search) is api.BatchResult
    nbest, crf_nbest = fcd.beam_search_nbest_batch_raw(x, 2, 5, 0.0), fcd.crf_beam_search_nbest_batch_raw(xc, init, 2, 5, 0.0)
    assert not nbest.crf and crf_nbest.crf
    return {
        "plain": plain, "crf search": crf_search, "crf": crf, "nbest": nbest, "crf nbest": crf_nbest,
        "plain without path": api.BatchResult(plain.labels, None, plain.out_len, plain.status),
        "crf without path": api._CrfBatchResult(crf.labels, None, crf.out_len, crf.status),
        "nbest without path": api.NBestResult(nbest.labels, None, nbest.out_len, nbest.score, nbest.n_hyp, nbest.status),
        "crf nbest without path": api.NBestResult(crf_nbest.labels, None, crf_nbest.out_len, crf_nbest.score,
                                                  crf_nbest.n_hyp, crf_nbest.status, crf=True),
    }


BATCH_BAND = "a band needs the result's path"
RAW_BAND = "a band needs paths"
# (result, family of methods, posteriors given, band) -> None: the call goes through, else (exception, its message)
METHOD_TABLE = [
    ("plain", "ctc", "ctc", 0, None),
    ("plain", "ctc", "ctc", 2, None),
    ("plain", "ctc", "crf", 0, (ValueError, "covers the plain CTC searches")),
    ("plain", "crf", "ctc", 0, (ValueError, "covers the results of the CRF searches")),
    ("plain", "crf", "crf", 0, None),  # BatchResult.crf_* looks at the posteriors' rank alone
    ("crf search", "crf", "crf", 2, None),
    ("crf search", "ctc", "ctc", 0, None),  # ... and BatchResult.ctc_* at the result's class
    ("crf", "ctc", "ctc", 0, (ValueError, "covers the plain CTC searches")),
    ("crf", "crf", "crf", 0, None),
    ("crf", "crf", "crf", 2, None),
    ("crf", "crf", "ctc", 0, (ValueError, "covers the results of the CRF searches")),
    ("nbest", "ctc", "ctc", 0, None),
    ("nbest", "ctc", "ctc", 2, None),
    ("nbest", "ctc", "crf", 0, (ValueError, "covers the plain CTC searches")),
    ("nbest", "crf", "crf", 0, (ValueError, "covers the results of the CRF searches")),  # NBestResult.crf_* asks self.crf too
    ("crf nbest", "crf", "crf", 0, None),
    ("crf nbest", "crf", "crf", 2, None),
    ("crf nbest", "crf", "ctc", 0, (ValueError, "covers the results of the CRF searches")),
    ("crf nbest", "ctc", "ctc", 0, (ValueError, "covers the plain CTC searches")),
    # a band on a result without a path: BatchResult refuses it itself, NBestResult leaves it to the batch call
    ("plain without path", "ctc", "ctc", 0, None),
    ("plain without path", "ctc", "ctc", 2, (ValueError, BATCH_BAND)),
    ("plain without path", "crf", "crf", 2, (ValueError, BATCH_BAND)),
    ("crf without path", "crf", "crf", 0, None),
    ("crf without path", "crf", "crf", 2, (ValueError, BATCH_BAND)),
    ("nbest without path", "ctc", "ctc", 0, None),
    ("nbest without path", "ctc", "ctc", 2, (ValueError, RAW_BAND)),
    ("crf nbest without path", "crf", "crf", 0, None),
    ("crf nbest without path", "crf", "crf", 2, (ValueError, RAW_BAND)),
    # the refusal of the result's kind comes before the one of the band
    ("crf without path", "ctc", "ctc", 2, (ValueError, "covers the plain CTC searches")),
    ("nbest without path", "crf", "crf", 2, (ValueError, "covers the results of the CRF searches")),
]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which,family,given,band,refusal", METHOD_TABLE,
                         ids=["%s.%s_* on %s posteriors, band %d" % row[:4] for row in METHOD_TABLE])
def test_result_method(fcd, results, kind, which, family, given, band, refusal):
    method = getattr(results[which], "%s_%s" % (family, kind))
    args = (posteriors(given),) + ((np.ones((B, S), np.float32),) if family == "crf" else ())
    if refusal is None:
        got = method(*args, band=band)
        logp = got if isinstance(got, np.ndarray) else got.logp
        assert logp.shape == (B, 2 if "nbest" in which else 1)
    else:
        with pytest.raises(refusal[0], match=refusal[1]):
            method(*args, band=band)


# ---- the wide switch --------------------------------------------------------------------------
WIDE_CALLS = [("ctc", "occupancy"), ("crf", "score"), ("crf", "occupancy")]


def wide_call(fcd, model, kind, t, n, **kw):
    """no reads at all: the library checks the shapes against its limits and launches nothing"""
    x = np.zeros((0, t, S, n) if model == "crf" else (0, t, n), np.float32)
    head = (x, np.ones((0, S), np.float32)) if model == "crf" else (x,)
    return getattr(fcd, "%s_%s_batch_raw" % (model, kind))(*head, np.zeros((0, t), np.uint8), np.zeros(0, np.uint32), **kw)


@pytest.mark.parametrize("model,kind", WIDE_CALLS, ids=["%s_%s" % c for c in WIDE_CALLS])
def test_wide_call_that_raises_leaves_the_switch_off(fcd, model, kind):
    from fast_ctc_decode_amd import _native as nat
    over = 600  # rows and labels: a window of 1201 (CTC) / 601 (CRF) states, beyond what wide=False takes
    with pytest.raises(nat.NativeError) as e:
        wide_call(fcd, model, kind, over, N)
    assert e.value.code == nat.E_UNSUPPORTED
    wide_call(fcd, model, kind, over, N, wide=True)
    with pytest.raises(nat.NativeError):  # (the switch was taken back behind that call as well)
        wide_call(fcd, model, kind, over, N)
    with pytest.raises(nat.NativeError) as e:
        wide_call(fcd, model, kind, over, 10, wide=True)  # more than 8 labels: refused inside the library, wide or not
    assert e.value.code == nat.E_UNSUPPORTED
    with pytest.raises(nat.NativeError) as e:
        wide_call(fcd, model, kind, over, N)
    assert e.value.code == nat.E_UNSUPPORTED and "states" in str(e.value)
