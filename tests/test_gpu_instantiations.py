"""Every row of the instantiation ledger (tests/instantiation_cases.py) on the MI355X: numpy inputs through the _host entry
points (device tensors where the entry point takes device pointers), each against its reference -- exactly for the
searches, within the case files' tolerances for the lattice walks.

The device cannot say which kernel ran.  That a row selects the instantiation it is named after is established on the
CPU, from the emulator's launch log (tests/test_instantiation_ledger_emu.py), for the same host dispatch code: the
ledger's docstring lists every FCD_HIPEMU branch of it, and none changes the choice.

One test per family slice (a wave shape, a lane alphabet, a template), so that each takes a few seconds; a slice runs all
of its rows and reports every one that failed."""
import pytest

import instantiation_cases as IC

pytestmark = pytest.mark.gpu


def _slice_of(name):
    template, args = IC.parse(name)
    if template == "beam_wave_kernel":
        return "wave N%d GW%d RPW%d S%d" % args[:4]
    if template == "beam_lane_kernel":
        return "lane %s" % ("crf" if args[3] else "N%d" % args[0])
    return template.replace("_kernel", "")


SLICES = {}
for _name, _, _ in IC.rows():
    SLICES.setdefault(_slice_of(_name), []).append(_name)


@pytest.fixture(scope="module")
def fcd():
    import fast_ctc_decode_amd as m
    return m


def test_every_row_is_in_a_slice():
    assert sum(len(v) for v in SLICES.values()) == len(IC.rows()) == len({n for n, _, _ in IC.rows()})


@pytest.mark.parametrize("which", sorted(SLICES))
def test_rows(fcd, which):
    failed = []
    for name in SLICES[which]:
        try:
            IC.run(fcd, name, device="cuda")
        except AssertionError as e:
            failed.append((name, str(e)[:400]))
    assert not failed, "%d of %d rows failed: %s" % (len(failed), len(SLICES[which]), failed)
