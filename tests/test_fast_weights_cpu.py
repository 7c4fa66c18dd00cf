"""The CPU yardstick of RPF_FLAG_FAST_WEIGHTS (tests/fast_weights_ref.py) against the oracle, no GPU: on the nine 19-dim frames
of tests/planted_nbhd.py, both sigma seeds, EPS policy, on the check set (every pixel of the target row, which holds all
targets),

  * the fp64 form of the restatement IS the oracle's stage 4: colours within 1e-12 relative L2 (rounding: another order of
    the sums, one exp of the summed exponent);
  * the fp32 form -- the arithmetic the flag documents -- lies e32 from the oracle, 0 < e32 <= 1e-6 at the active seed: the
    GPU's regression bar 16 * e32 (tests/test_fast_weights_gpu.py) then stays below 1.6 % of the 1e-4 contract.

Measured (relative L2 on the check set):

  frame   fp64 form, active seed   fp32 form, active seed (frame | worst pixel)
  U8      5.1e-16                  1.24e-08 | 2.64e-08
  U2      3.4e-16                  7.8e-09  | 1.83e-08
  U3      7.2e-16                  9.5e-09  | 2.13e-08
  U12     5.6e-16                  1.19e-08 | 1.81e-08
  B16     9.1e-16                  1.00e-08 | 1.84e-08
  B32     1.4e-15                  8.9e-09  | 1.44e-08
  B64     2.2e-15                  8.4e-09  | 1.19e-08
  B40     2.6e-15                  7.6e-09  | 9.2e-09
  B17     2.3e-15                  7.9e-09  | 1.21e-08

At the reference's seed both forms are exactly 0 from the oracle on all nine: the filter is the identity there (every weight
but a sample's own underflows, in fp32 as in fp64).
"""
import numpy as np
import pytest

import fast_weights_ref as R
import planted_nbhd as P

FRAMES19 = [f for f, v in P.FRAMES.items() if v[0] == (2, 12, "f32")]
SEEDS = pytest.mark.parametrize("seed", [0.002, P.ACTIVE_SIGMA_SEED], ids=["ref_seed", "active_seed"])


def test_the_nine_19_dim_frames():
    assert FRAMES19 == ["U8", "U2", "U3", "U12", "B16", "B32", "B64", "B40", "B17"]


@SEEDS
@pytest.mark.parametrize("fid", FRAMES19)
def test_fp64_form_is_the_oracles_stage_4(oracle, fid, seed):
    e64 = R.row_distance(oracle, fid, R.EPS, seed, np.float64)
    print("%s seed %g: fp64 form vs oracle %.3e" % (fid, seed, e64))
    assert e64 <= 1e-12, e64


@SEEDS
@pytest.mark.parametrize("fid", FRAMES19)
def test_fp32_form_distance_from_the_oracle(oracle, fid, seed):
    e32 = R.row_distance(oracle, fid, R.EPS, seed, np.float32)
    b = (P.FRAMES[fid][2] - 1) // 2
    ref = P.oracle_pass(oracle, fid, R.EPS, seed)["colour"][:, b]
    got = R.target_row(oracle, fid, R.EPS, seed, np.float32)
    worst = max(R.rel_l2(got[:, x], ref[:, x]) for x in range(ref.shape[1]))
    print("%s seed %g: fp32 form vs oracle %.3e (worst pixel %.3e)" % (fid, seed, e32, worst))
    assert e32 <= 1e-6, e32
    if seed == P.ACTIVE_SIGMA_SEED:
        assert e32 > 0      # the weights are of order one: fp32 arithmetic shows
        cin = P.frame(fid)[1][2:5, b].astype(np.float64)
        assert R.rel_l2(ref, cin) > 0.05    # ... on colours that the pass moves
