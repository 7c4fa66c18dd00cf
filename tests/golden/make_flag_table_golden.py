#!/usr/bin/env python3
"""Generates tests/golden/flag_table.npz: what rpf_layout_kernels answers for every flag word and a set of sample layouts.

    python tests/golden/make_flag_table_golden.py          (needs the built library, no GPU; a second)

The fixture is a recording of the library's own answers, not of an oracle: it pins the refusals of rpf::layout_kernels
(csrc/rpf_api.hip) so that a change to the rule table there cannot move an answer unnoticed.  It was recorded from the library of
commit 0a8c4a5, before the refusals became a table, and is regenerated only when a flag or a refusal is added on purpose.

    flags    int32 [2048]      every word of the eleven RPF_FLAG_* bits, 0 .. 2047
    layouts  int32 [10][3]     (n_random, n_feat, plane_dtype) of tests/test_flag_table_cpu.py's LAYOUTS, in that order
    status   int32 [10][2048]  RPF_OK or RPF_E_UNSUPPORTED
    generic  int32 [10][2048]  *generic_out: 0 the compiled fused kernels, 1 the layout-generic ones, -1 where refused

Fixtures are data only: recorded answers.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import rpf_pkg  # noqa: E402

rpf_pkg.load()
from raytracer_rpf_amd import hip  # noqa: E402

N_FLAG_BITS = 11
# the two compiled layouts by their default and by name, fp16 / fp32 swapped, three layouts only the generic kernels take, two
# outside RPF_MAX_NDIM / the plane types
LAYOUTS = [(0, 0, 0), (2, 12, 0), (4, 18, 1), (4, 18, 0), (2, 12, 1), (3, 7, 0), (1, 1, 0), (8, 27, 1), (9, 27, 0), (0, 0, 2)]


def table():
    """(status, generic) int32 [len(LAYOUTS)][2 ** N_FLAG_BITS] of the loaded library"""
    status = np.empty((len(LAYOUTS), 1 << N_FLAG_BITS), np.int32)
    generic = np.empty_like(status)
    for i, (nr, nf, dt) in enumerate(LAYOUTS):
        for flags in range(1 << N_FLAG_BITS):
            st, g = hip.layout_kernels(hip.make_desc(8, 8, 4, flags=flags, n_random=nr, n_feat=nf, plane_dtype=dt))
            status[i, flags] = st
            generic[i, flags] = -1 if g is None else g
    return status, generic


if __name__ == "__main__":
    status, generic = table()
    ok0 = int(((status == hip.OK) & (generic == 0)).sum())
    ok1 = int(((status == hip.OK) & (generic == 1)).sum())
    refused = int((status == hip.E_UNSUPPORTED).sum())
    assert ok0 + ok1 + refused == status.size, "a status other than RPF_OK / RPF_E_UNSUPPORTED"
    path = os.path.join(HERE, "flag_table.npz")
    np.savez_compressed(path, flags=np.arange(1 << N_FLAG_BITS, dtype=np.int32), layouts=np.array(LAYOUTS, np.int32), status=status,
                        generic=generic)
    print("%s: %d bytes; (OK, 0) x %d, (OK, 1) x %d, RPF_E_UNSUPPORTED x %d" % (path, os.path.getsize(path), ok0, ok1, refused))
