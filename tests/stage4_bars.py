"""The per-sample bar of stage 4 (the S x N pair weights and the blend): how far one filtered colour of an fp64 kernel may lie
from the fp64 numpy restatement of tests/fast_weights_ref.py evaluated on the same stage 1 to 3 outputs.  A plain helper
module (like planted_nbhd.py): tests/test_stage4_per_sample_cpu.py guards the derivation against the oracle,
tests/test_stage4_per_sample_gpu.py holds every route's colours to it.  The bars are worst-case bounds, derived here; none is
fitted to what a kernel gives.

With u = 2^-53, nwt = 5 + n_feat weighted columns (pFilm 2, colour 3, the features), Nmax the largest neighbourhood among the
checked pixels and cmax the largest finite |colour_in| of the frame:

    delta_direct   = u * (745 * (nwt + 3) + 2 + Nmax)
    delta_expanded = delta_direct + u * 16 * nwt * czmax * Nmax
    czmax          = max(1 / (2 sigma_seed^2), 1 / (2 sigma_p^2))
    per-sample bar = 4 * delta * cmax

delta bounds the relative error of one pair weight w_ij = exp(-E_ij), E_ij = sum_k cz_k (z_ik - z_jk)^2, and of the two sums
over the neighbourhood it enters:

  exponent      z = (x - M) / SD is formed with an IEEE division from the same bits on both sides (the direct kernels).  A weight
                is non-zero only for E <= 745 (exp(-745.13) is the last denormal).  E is a sum of nwt non-negative terms of
                three roundings each (the difference, the square, the product with cz_k) plus the roundings of the sum: its
                absolute error is at most 745 * (nwt + 3) * u, which is the relative error of exp(-E) it causes.
  exp, sums     one exponential costs 2 u; each of the two sums over N terms (sum w, sum w c) costs N u, of which the quotient
                sees the difference: N u + 2 u.  (The generic kernels multiply three exponentials as the reference does -- 6 u
                and two products where this says 2 u; against 745 * (nwt + 3) that is below 0.1 % of the bar and inside the
                slack of the first term, whose three partial sums never reach 745 each.)
  expanded      the fused kernels evaluate E = A_i + B_j + sum_k u_ik z_jk, which cancels between
                A_i + B_j and the dot product: each of the nwt terms carries about 4 u cz_k (|z_ik| + |z_jk|)^2 <=
                16 u cz_k max z^2, and z^2 < N for a sample of a population of N (no sample lies more than sqrt(N - 1)
                standard deviations from its population's mean).  That holds for the exact SD of the population.  An SD
                taken from a variance E[x^2] - mean^2 that has cancelled (scene-scale magnitudes: tests/scene_scale.py) does
                not have to obey it, so the bound on z^2 is an argument, z2max: by default N, on such frames the largest z^2
                measured over the checked members from the oracle's mean and SD (tests/test_scene_scale_cpu.py).
                The fused kernels also form z as (x - M) * (1 / SD), two roundings more than the division: a relative 2 u on
                z_i and z_j moves cz_k (z_ik - z_jk)^2 by up to 4 u cz_k (|z_ik| + |z_jk|)^2, a second term of the same form.
                It is not budgeted separately: z^2 < N is attained by one sample of a population at most (z is of order one
                by construction), and the fused routes measure five orders or more below this bar.  Should
                a kernel ever come near, that term is the first to add.
  sigma         cz_k = weight_k / (2 sigma^2) with weight_k <= 1 (alpha, beta are products of terms 1 - W, W in [0, 1]);
                sigma_c^2 = sigma_f^2 = seed^2 / (1 - W_r_c)^2 >= seed^2, sigma_p = box // 4.
  to colours    the output is a convex combination sum_j w_j c_j / sum_j w_j: a relative error delta in every weight moves it
                by at most 2 delta times the range of the c_j, and the range is at most 2 cmax.

Which form a kernel uses, read from its source (csrc/):

  expanded   rpf_filter_impl.inc (every fused kernel: routes 0, 1, 2; one-wave, size-binned, four-wave, split, d19 and d27)
             and rpf_packed_impl.inc (the packed small-neighbourhood kernels of the same routes): both form the own rows
             u_i | A_i once and run one FMA per column and pair.
  direct     generic::filter_pixel_kernel (rpf_generic.hip: route 3, the streaming size class N > 3136 and the REF_ABORT redo
             list of every route) and generic::filter_wide_kernel (rpf_generic_wide.hip), whose stage 4 is one text,
             rpf_generic_stream_stages.inc; generic::filter_packed_kernel (rpf_generic_packed.hip) and
             generic::filter_wave_kernel (rpf_generic_wave.hip): routes 4, 5, 6, 7.  All four run
             sp / sc / sf term by term, (z_i - z_j)^2 * weight, as rpf.cpp:646-670.

Values: direct at nwt = 17, Nmax = 3136: 8e-12 cmax.  Expanded at seed 0.5: 5e-11 (Nmax 392) ... 4e-10 (Nmax 3136); at seed
0.05 a hundred times that; at the reference's seed 0.002 the expanded bar is 1e-6 and useless, so the checks run at active
seeds only."""
import numpy as np

U = 2.0 ** -53
MAX_EXPONENT = 745          # exp(-E) == 0.0 beyond it
RESIDENT = 3136             # fused routes: neighbourhoods above it run on generic::filter_pixel_kernel (direct)

# route (rpf_query_route) -> form of the kernels that filter its resident pixels
ROUTE_FORM = {0: "expanded", 1: "expanded", 2: "expanded", 3: "direct", 4: "direct", 5: "direct", 6: "direct", 7: "direct"}


def delta(form, nwt, nmax, sigma_seed, box, z2max=None):
    """relative error bound of the pair weights and their sums; z2max: a bound on z^2 over the checked members for the expanded
    form (None: nmax, from z^2 < N)"""
    d = U * (MAX_EXPONENT * (nwt + 3) + 2 + nmax)
    if form == "direct":
        return d
    if form != "expanded":
        raise ValueError(form)
    sigma_p = float(box // 4)
    czmax = 1.0 / (2 * sigma_seed * sigma_seed)
    if sigma_p > 0:
        czmax = max(czmax, 1.0 / (2 * sigma_p * sigma_p))
    return d + U * 16 * nwt * czmax * (nmax if z2max is None else z2max)


def sample_bar(form, n_feat, nmax, sigma_seed, box, z2max=None):
    """the per-sample bar relative to cmax: |colour - restatement| <= sample_bar(...) * cmax"""
    return 4 * delta(form, 5 + n_feat, int(nmax), sigma_seed, box, z2max)


def cmax_of(colour_in):
    """the largest finite |colour_in| of a frame"""
    c = np.abs(np.asarray(colour_in, np.float64))
    return float(c[np.isfinite(c)].max())


def worst_sample(got, ref):
    """max |got - ref| over the entries where both are finite (0.0 where there is none)"""
    m = np.isfinite(got) & np.isfinite(ref)
    return float(np.abs(got[m] - ref[m]).max()) if m.any() else 0.0
