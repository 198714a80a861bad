"""The public surface of the labelling-lattice calls (fast_ctc_decode_amd/api.py: score, align, posterior, edits and
occupancy, CTC and CRF, batch and single read, and the results' methods): the signatures and the docstrings of the module's
functions as they stood before the ten call bodies became one, and the package's exports.  Nothing here loads the library."""
import hashlib
import inspect

import pytest

import fast_ctc_decode_amd as fcd
from fast_ctc_decode_amd import api

CTC_BATCH = ("(network_outputs, labels, label_lengths, collapse_repeats=True, lengths=None, paths=None, band=0, n_valid=None, "
             "input_dtype=None, handle=None)")
CRF_BATCH = ("(network_outputs, init_states, labels, label_lengths, lengths=None, paths=None, band=0, n_valid=None, "
             "input_dtype=None, handle=None)")
OCC_TAIL = ("n_valid=None, out=None, scale=1.0, accumulate=False, time_major_out=False, input_dtype=None, handle=None, "
            "wide=False)")
CTC_ONE = "(network_output, sequence, alphabet, collapse_repeats=True)"
CRF_ONE = "(network_output, init_state, sequence, alphabet)"

SIGNATURES = {
    "ctc_score_batch_raw": CTC_BATCH,
    "ctc_align_batch_raw": CTC_BATCH,
    "ctc_posterior_batch_raw": CTC_BATCH,
    "ctc_edits_batch_raw": CTC_BATCH,
    "ctc_occupancy_batch_raw": CTC_BATCH.replace("n_valid=None, input_dtype=None, handle=None)", OCC_TAIL),
    "crf_score_batch_raw": CRF_BATCH[:-1] + ", wide=False)",
    "crf_align_batch_raw": CRF_BATCH,
    "crf_posterior_batch_raw": CRF_BATCH,
    "crf_edits_batch_raw": CRF_BATCH,
    "crf_occupancy_batch_raw": CRF_BATCH.replace("n_valid=None, input_dtype=None, handle=None)", OCC_TAIL),
    "ctc_score": CTC_ONE,
    "ctc_align": CTC_ONE,
    "ctc_posterior": CTC_ONE,
    "ctc_edits": CTC_ONE,
    "ctc_occupancy": CTC_ONE[:-1] + ", wide=False)",
    "crf_score": CRF_ONE[:-1] + ", wide=False)",
    "crf_align": CRF_ONE,
    "crf_posterior": CRF_ONE,
    "crf_edits": CRF_ONE,
    "crf_occupancy": CRF_ONE[:-1] + ", wide=False)",
}

CTC_METHOD = "(self, network_outputs, collapse_repeats=True, lengths=None, band=0, input_dtype=None)"
CRF_METHOD = "(self, network_outputs, init_states, lengths=None, band=0, input_dtype=None)"
METHODS = {
    "ctc_score": CTC_METHOD,
    "ctc_align": CTC_METHOD,
    "ctc_posterior": CTC_METHOD,
    "ctc_edits": CTC_METHOD,
    "ctc_occupancy": CTC_METHOD[:-1] + ", wide=False)",
    "crf_score": CRF_METHOD[:-1] + ", wide=False)",
    "crf_align": CRF_METHOD,
    "crf_posterior": CRF_METHOD,
    "crf_edits": CRF_METHOD,
    "crf_occupancy": CRF_METHOD[:-1] + ", wide=False)",
}

DOC_SHA1 = {
    "ctc_score_batch_raw": "aa72c286ab02487b4ff23f4fe3e2071c083e4b9d",
    "ctc_align_batch_raw": "ebfc29dd0cad6d4387441d441c347ea0ed9a9535",
    "ctc_posterior_batch_raw": "eb11acdd661523253172ccef737df9d4aae8b91e",
    "ctc_edits_batch_raw": "c5007bc7c77aea0c3a2cf050bd63ec96f8c98e1f",
    "ctc_occupancy_batch_raw": "92fed12ac3399e1c2196fe949bce71cd2045d95f",
    "crf_score_batch_raw": "7c5ceeff283d58576c5890cef9cf407353f3c355",
    "crf_align_batch_raw": "f7a0874f1d0a6fe60c7f71d46f3469be015f9872",
    "crf_posterior_batch_raw": "a992a662b2794381de95076bb51b21a1c19ea89d",
    "crf_edits_batch_raw": "c859b82ac7305e82c09bc21016eee5931fc60289",
    "crf_occupancy_batch_raw": "479cb00e556b16b77a4d6e8e24d10db29db169e5",
    "ctc_score": "f86db3077ae19366080d29b6653b59b4f476f83a",
    "ctc_align": "68e35d518983e5b6084f977147294518cb946ac9",
    "ctc_posterior": "7ad253d9910444d64797c9140a4b34fc9c17c3d2",
    "ctc_edits": "b148f03d20096f859a54b62a6fc2daf52f43483b",
    "ctc_occupancy": "dd5f3d0a02b631ccb87d7d9dc53463a0231ccec4",
    "crf_score": "02aab88f522c3591d1ca7c877cdbb31ac2afdd58",
    "crf_align": "e887052c8b9117b09ac5e18a5ee9a3784078147e",
    "crf_posterior": "8ff384d7d27decefbab03743705320fe93ad7842",
    "crf_edits": "54688afe494ecad0a420bf29df3e000108935f6c",
    "crf_occupancy": "86cd667f48bbbc0daa842a5e62873c795fad7929",
}

# what `from fast_ctc_decode_amd import ...` offered from api.py before the change
EXPORTS = """BatchResult BeamSearchSession CrfBeamSearchSession NBestResult MarginalResult TransitionResult __version__
beam_search beam_search_batch beam_search_batch_raw beam_search_duplex beam_search_duplex_batch beam_search_duplex_batch_raw
beam_search_nbest beam_search_nbest_batch_raw set_duplex_logadd_mode set_tie_order tie_order set_overlap overlap_join
set_coalescing coalescing_stats crf_beam_search crf_beam_search_batch crf_beam_search_batch_raw crf_beam_search_duplex
crf_beam_search_duplex_batch crf_beam_search_duplex_batch_raw crf_beam_search_nbest crf_beam_search_nbest_batch_raw
crf_greedy_search crf_viterbi_search crf_viterbi_search_batch crf_viterbi_search_batch_raw crf_transition_probs
crf_transition_probs_batch_raw crf_marginals crf_marginals_batch_raw crf_logz crf_align crf_align_batch_raw crf_posterior
crf_edits crf_edits_batch_raw crf_posterior_batch_raw crf_occupancy ctc_occupancy ctc_occupancy_batch_raw ctc_loss
crf_occupancy_batch_raw crf_ctc_loss OccupancyResult crf_score crf_score_batch_raw AlignResult ctc_align ctc_align_batch_raw
EditResult ctc_edits ctc_edits_batch_raw PosteriorResult ctc_posterior ctc_posterior_batch_raw ctc_score ctc_score_batch_raw
crf_greedy_search_batch crf_greedy_search_batch_raw estimate_envelope estimate_envelope_batch viterbi_search
viterbi_search_batch viterbi_search_batch_raw""".split()


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_function_signature_and_docstring(name):
    f = getattr(api, name)
    assert str(inspect.signature(f)) == SIGNATURES[name]
    assert hashlib.sha1(f.__doc__.encode()).hexdigest() == DOC_SHA1[name]


@pytest.mark.parametrize("cls", (api.BatchResult, api.NBestResult), ids=lambda c: c.__name__)
@pytest.mark.parametrize("name", sorted(METHODS))
def test_result_method_signature(cls, name):
    method = getattr(cls, name)
    assert str(inspect.signature(method)) == METHODS[name]
    # (the methods' docstrings merged: each still says what it returns for a plain and for an n-best result)
    assert "n_reads, 1" in method.__doc__ and "n_reads, n_best" in method.__doc__


def test_package_exports():
    assert len(SIGNATURES) == 20 and set(SIGNATURES) <= set(EXPORTS)
    for name in EXPORTS:
        assert getattr(fcd, name) is getattr(api, name), name
