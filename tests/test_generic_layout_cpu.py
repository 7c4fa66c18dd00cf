"""The layout-generic route's device-free surface: rpf_layout_kernels' truth table (what the filter entry points answer
about a descriptor's layout and flags, without a context) and the constants the header, the binding and the oracle share."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(path, name):
    with open(os.path.join(ROOT, path)) as f:
        m = re.search(r"\b%s\s*(?:=\s*)?(\d+)" % name, f.read())
    assert m, (path, name)
    return int(m.group(1))


def test_flag_and_max_ndim_match_the_headers(hipmod):
    assert hipmod.FLAG_GENERIC == _header("include/rpf_hip.h", "RPF_FLAG_GENERIC") == 8
    assert hipmod.MAX_NDIM == _header("include/rpf_hip.h", "RPF_MAX_NDIM") == 40
    assert _header("include/rpf_hip.h", "RPF_MAX_NDIM") == _header("oracle/rpf_oracle.h", "RPF_O_MAXDIM")
    # the flag is a bit of its own
    assert hipmod.FLAG_GENERIC & (hipmod.FLAG_TIMING | hipmod.FLAG_FAST_WEIGHTS | hipmod.FLAG_NO_OVERLAP) == 0


@pytest.mark.parametrize("lay,flags,want", [
    (dict(), 0, ("OK", 0)),                                                      # the reference's 19 dims: compiled kernels
    (dict(), "G", ("OK", 1)),                                                    # ... on the generic kernels by request
    (dict(n_random=4, n_feat=18, plane_dtype=1), 0, ("OK", 0)),                  # the 27 dims on fp16 planes: compiled kernels
    (dict(n_random=4, n_feat=18, plane_dtype=1), "G", ("OK", 1)),
    (dict(n_random=4, n_feat=18, plane_dtype=0), 0, ("E_UNSUPPORTED", None)),    # the refusal stays without the flag
    (dict(n_random=4, n_feat=18, plane_dtype=0), "G", ("OK", 1)),
    (dict(n_random=2, n_feat=18, plane_dtype=1), 0, ("E_UNSUPPORTED", None)),
    (dict(n_random=1, n_feat=1), "G", ("OK", 1)),                                # 7 dims, the narrowest
    (dict(n_random=8, n_feat=27), "G", ("OK", 1)),                               # 40 dims, the widest
    (dict(n_random=9, n_feat=27), "G", ("E_UNSUPPORTED", None)),                 # 41 dims
    (dict(n_random=-1, n_feat=3), "G", ("E_UNSUPPORTED", None)),
    (dict(plane_dtype=2), "G", ("E_UNSUPPORTED", None)),                         # no such plane type
    (dict(), "GF", ("E_UNSUPPORTED", None)),                                     # the generic kernels are fp64 throughout
    (dict(n_random=3, n_feat=7), "GF", ("E_UNSUPPORTED", None)),
    (dict(), "GT", ("OK", 1)),                                                   # the other flags do not matter
    (dict(), "F", ("OK", 0)),                                                    # fp32 pair weights: the reference's 19 dims only
    (dict(n_random=4, n_feat=18, plane_dtype=1), "F", ("E_UNSUPPORTED", None)),  # ... no 27-dim instantiation of them exists
    (dict(n_random=4, n_feat=18, plane_dtype=1), "FT", ("E_UNSUPPORTED", None)),
])
def test_layout_kernels_truth_table(hipmod, lay, flags, want):
    bits = {"G": hipmod.FLAG_GENERIC, "F": hipmod.FLAG_FAST_WEIGHTS, "T": hipmod.FLAG_TIMING}
    fl = sum(bits[c] for c in flags) if flags else 0
    st, generic = hipmod.layout_kernels(hipmod.make_desc(8, 8, 4, flags=fl, **lay))
    assert (st, generic) == (getattr(hipmod, want[0]), want[1])


def test_layout_kernels_null_desc_and_null_out(hipmod):
    import ctypes as C
    assert hipmod.layout_kernels(None) == (hipmod.E_BADARG, None)
    L = hipmod.load()
    d = hipmod.make_desc(8, 8, 4, flags=hipmod.FLAG_GENERIC, n_random=3, n_feat=7)
    assert L.rpf_layout_kernels(C.byref(d), None) == hipmod.OK               # generic_out may be NULL
    assert hipmod.status_string(hipmod.E_UNSUPPORTED) == "RPF_E_UNSUPPORTED"
