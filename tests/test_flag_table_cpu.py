"""rpf_layout_kernels over every flag word: the answers of the refusal table in rpf::layout_kernels (csrc/rpf_api.hip) against
tests/golden/flag_table.npz, recorded from the library of before the refusals were a table (tests/golden/make_flag_table_golden.py).
2048 flag words (all eleven RPF_FLAG_* bits) x ten layouts (n_random, n_feat, plane_dtype); no device needed.

The recording's own totals are asserted too, so that a regenerated fixture cannot quietly carry other answers: per layout
(OK, 0) / (OK, 1) / refused are 48 / 176 / 1824 for the reference layout (by default and by name), 40 / 176 / 1832 for (4, 18, f16)
(RPF_FLAG_FAST_WEIGHTS exists for the 19 dims only), 0 / 176 / 1872 for the five layouts only the generic kernels take, and 2048
refusals for the two layouts outside RPF_MAX_NDIM and the plane types."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flag_table.npz")
N_FLAG_BITS = 11
LAYOUTS = [(0, 0, 0), (2, 12, 0), (4, 18, 1), (4, 18, 0), (2, 12, 1), (3, 7, 0), (1, 1, 0), (8, 27, 1), (9, 27, 0), (0, 0, 2)]
PER_LAYOUT = [(48, 176, 1824)] * 2 + [(40, 176, 1832)] + [(0, 176, 1872)] * 5 + [(0, 0, 2048)] * 2


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    assert g["layouts"].tolist() == [list(lay) for lay in LAYOUTS]
    assert g["flags"].tolist() == list(range(1 << N_FLAG_BITS))
    return {k: g[k] for k in ("status", "generic")}


def counts(hipmod, status, generic):
    return (int(((status == hipmod.OK) & (generic == 0)).sum()), int(((status == hipmod.OK) & (generic == 1)).sum()),
            int((status == hipmod.E_UNSUPPORTED).sum()))


def test_the_flag_bits_are_the_eleven_of_the_header(hipmod):
    names = [n for n in dir(hipmod) if n.startswith("FLAG_")]
    assert sorted(getattr(hipmod, n) for n in names) == [1 << k for k in range(N_FLAG_BITS)], names


def test_recording_totals(hipmod, gold):
    assert counts(hipmod, gold["status"], gold["generic"]) == (136, 1408, 18936)
    for i, want in enumerate(PER_LAYOUT):
        assert counts(hipmod, gold["status"][i], gold["generic"][i]) == want, LAYOUTS[i]
    assert ((gold["generic"] == -1) == (gold["status"] != hipmod.OK)).all()


@pytest.mark.parametrize("lay", range(len(LAYOUTS)), ids=["%d-%d-%d" % lay for lay in LAYOUTS])
def test_every_flag_word_answers_as_recorded(hipmod, gold, lay):
    nr, nf, dt = LAYOUTS[lay]
    status = np.empty(1 << N_FLAG_BITS, np.int32)
    generic = np.empty_like(status)
    for flags in range(1 << N_FLAG_BITS):
        st, g = hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=flags, n_random=nr, n_feat=nf, plane_dtype=dt))
        status[flags], generic[flags] = st, (-1 if g is None else g)
    bad = np.flatnonzero((status != gold["status"][lay]) | (generic != gold["generic"][lay]))
    assert bad.size == 0, [(int(f), int(status[f]), int(generic[f]), int(gold["status"][lay][f]), int(gold["generic"][lay][f])) for f in bad[:8]]


def test_timing_no_overlap_and_spike_clamp_never_change_an_answer(hipmod, gold):
    flags = np.arange(1 << N_FLAG_BITS)
    for bit in (hipmod.FLAG_TIMING, hipmod.FLAG_NO_OVERLAP, hipmod.FLAG_SPIKE_CLAMP):
        for k in ("status", "generic"):
            assert (gold[k][:, flags] == gold[k][:, flags & ~bit]).all(), (bit, k)
