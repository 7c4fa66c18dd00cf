"""ctypes binding of the C ABI declared in include/rpf_hip.h (librpf_hip.so).

This is the ONLY compute path of the package: if the library is missing the import of this module raises
(no CPU fallback, no oracle).  Host-buffer entry points take numpy arrays; device entry points take raw
device pointers (e.g. torch tensors' ``data_ptr()``), torch is used by callers only for HBM allocation,
streams and torch.distributed.
"""
import ctypes as C
import weakref
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RPF_HIP_LIB: load another build of the same ABI (profiling variants, scripts/ablate_mi.sh); default = the in-tree library
LIB_PATH = os.environ.get("RPF_HIP_LIB") or os.path.join(_HERE, "lib", "librpf_hip.so")

NDIM, NFEAT, NPAIR, MAX_BOXES = 19, 12, 96, 8
OK, E_BADARG, E_HIP, E_NONFINITE, E_NOMEM, E_UNSUPPORTED, E_NODEVICE = range(7)
BETA_REF_GCC11_O3, BETA_REF_GCC11_O2, BETA_PAPER = 0, 1, 2
DEGEN_REF_ABORT, DEGEN_EPS = 0, 1
FLAG_TIMING = 1
FLAG_FAST_WEIGHTS = 2
FLAG_NO_OVERLAP = 4
FLAG_GENERIC = 8  # the layout-generic kernels: required for a layout without compiled kernels, allowed for the two compiled ones
FLAG_GENERIC_PACKED = 16  # with FLAG_GENERIC: neighbourhoods of N <= 64 samples on the packed generic kernels (route 4)
FLAG_GENERIC_WAVE = 32  # with FLAG_GENERIC | FLAG_GENERIC_PACKED: 64 < N <= 832 on the one-wave generic kernels (route 5)
FLAG_WIDE_CLASSES = 128  # with FLAG_WIDE_NBHD: a wide pass counted first and dealt by size class (route 7; 6 for a pass with S > 832)
# with FLAG_GENERIC | FLAG_GENERIC_PACKED (with or without FLAG_GENERIC_WAVE): the pair weights of stage 4 in fp32 on the packed and
# one-wave generic kernels (routes 4 / 5 as without it; the rest list, the redo list and a route-3 pass stay fp64, same bits);
# refused without both flags, with FLAG_FAST_WEIGHTS (which keeps its meaning: the fused 19-dim kernels) and with FLAG_WIDE_NBHD
FLAG_GENERIC_FAST = 256
# with FLAG_GENERIC and / or FLAG_WIDE_NBHD: the pair weights of stage 4 in fp32 on the streaming generic kernel (route 3, the rest
# lists of routes 4 / 5) and on every kernel of a wide pass (routes 6 / 7); routes, launches and counters as without it; the redo
# list and every pass on the fused kernels stay fp64, same bits; refused without both flags (and, with FLAG_FAST_WEIGHTS, by one of
# that flag's refusals)
FLAG_STREAM_FAST = 512
# after the last pass of the call: the spike pass on the fp64 colours (spike clamp + energy preservation, DESIGN.md section 12;
# Context.set_spike / spike_stats), before the reduce, every download and the film step; independent of every route flag;
# filter_pass_debug refuses it
FLAG_SPIKE_CLAMP = 1024
# the published random-subset gather (Context.set_sampling): a pass with draws > 0 draws that many candidates per
# pixel instead of walking the box (route 8; fp64; S + draws <= 832, or SAMPLED_MAX with SAMPLED_REST_FLAG); a pass with draws == 0 runs as without the flag.  Refused
# without set_sampling, under DEGEN_REF_ABORT on a sampled pass, and with FLAG_FAST_WEIGHTS / FLAG_GENERIC_FAST / FLAG_STREAM_FAST.
# RPF_FLAG_SAMPLED_NBHD of the header.  Its name stands outside the FLAG_* family on purpose: that family is the eleven bits whose
# rpf_layout_kernels answers tests/golden/flag_table.npz records (words 0 .. 2047), and tests/test_flag_table_cpu.py holds it to
# exactly those; the twelfth bit has its own table in tests/test_sampled_cpu.py.  The name is provisional: once that test and its
# recording are widened to twelve bits, it becomes FLAG_SAMPLED_NBHD like the others
SAMPLED_NBHD_FLAG = 2048
# the published membership test (Context.set_membership): stage 1b takes a multiple of sigma and an absolute
# floor per feature, so that a flat pixel accepts its flat neighbours.  Every pass of the call: a full-box pass takes route 9 (count
# kernel, size classes, the wide kernel for N > 832; fp64), a sampled pass stays route 8 and tests its draws the same way.  Refused
# without set_membership, under DEGEN_REF_ABORT, with FLAG_FAST_WEIGHTS / FLAG_GENERIC_FAST / FLAG_STREAM_FAST, and on a full-box pass
# with S > 832.  RPF_FLAG_MEMBER_TEST of the header; the name stays outside the FLAG_* family for SAMPLED_NBHD_FLAG's reason (its
# table: tests/test_member_test_cpu.py)
MEMBER_TEST_FLAG = 4096
# modifies MEMBER_TEST_FLAG: a full-box pass of the call on a compiled layout (no FLAG_GENERIC, box*box*S <=
# 65535, not forced wide, no schedule gain other than 1) runs on the compiled kernels behind a count kernel under the configured
# test: route 10, route 2's structure, the same member lists as route 9.  Every other pass runs as without it.  Refused without
# MEMBER_TEST_FLAG.  RPF_FLAG_MEMBER_FUSED of the header; the name stays outside the FLAG_* family for MEMBER_TEST_FLAG's reason
# (its table: tests/test_member_fused_cpu.py)
MEMBER_FUSED_FLAG = 65536
# the per-pass schedule of the weight stage (Context.set_schedule): pass p of a call reads entry pass0 + p of
# a table of (seed, gain_c, gain_f); the seed stands for the descriptor's sigma_seed, and alpha_k = clamp0(1 - gain_c W_r^{c,k}),
# beta_k = clamp0(1 - gain_f W_r^{f,k}) W_c^{f,k}.  A pass with both gains 1 runs as without the flag on any route (the fused ones
# included) with its entry's seed; a pass with another gain needs a layout-generic route (FLAG_GENERIC, a wide pass, a sampled
# pass, MEMBER_TEST_FLAG) and DEGEN_EPS.  Selects no route.  RPF_FLAG_SCHEDULE of the header; the name stays outside the FLAG_*
# family for SAMPLED_NBHD_FLAG's reason (tests/test_flag_table_cpu.py holds FLAG_* to eleven bits)
SCHEDULE_FLAG = 8192
# modifies SCHEDULE_FLAG: a permission, not a route.  A pass with a gain other than 1 that carries no
# layout-generic bit runs on the route it takes with gains of 1 (0, 1 or 2) on the scheduled builds of the compiled kernels, and
# under MEMBER_TEST_FLAG | MEMBER_FUSED_FLAG it takes route 10 instead of 9; every other pass runs as without it.  Refused without
# SCHEDULE_FLAG, and with FLAG_FAST_WEIGHTS on such a pass (the scheduled builds are fp64).  RPF_FLAG_SCHEDULE_FUSED of the header;
# the name stays outside the FLAG_* family for SAMPLED_NBHD_FLAG's reason (its table: tests/test_schedule_fused_cpu.py)
SCHEDULE_FUSED_FLAG = 131072
# modifies SAMPLED_NBHD_FLAG: a sampled pass may have S + draws <= SAMPLED_MAX instead of 832; pixels that end
# with N > 832 go to a rest launch that reads their listed members (route 8 still); a pass with S + draws <= 832 runs as without it;
# max_draws() tells the bound.  Refused without SAMPLED_NBHD_FLAG.  RPF_FLAG_SAMPLED_REST of the header; the name stays outside the
# FLAG_* family for SAMPLED_NBHD_FLAG's reason (its table: tests/test_sampled_rest_cpu.py)
SAMPLED_REST_FLAG = 16384
SAMPLED_MAX = 8192  # RPF_SAMPLED_MAX
# modifies SAMPLED_NBHD_FLAG: a sampled pass of the call on a compiled layout (no FLAG_GENERIC, box*box*S <=
# 65535, not forced wide, S + draws <= 3136, no schedule gain other than 1 unless SCHEDULE_FUSED_FLAG, mask stride within option
# "sampled_fused_stride") runs on the compiled kernels behind a count kernel that leaves the draws as acceptance masks: route 11,
# route 2's class kernels, the same member lists as route 8.  Every other pass runs as without it.  Refused without
# SAMPLED_NBHD_FLAG.  RPF_FLAG_SAMPLED_FUSED of the header, hip.SAMPLED_FUSED_FLAG; the name stays outside the FLAG_* family for
# SAMPLED_NBHD_FLAG's reason (its table: tests/test_sampled_fused_cpu.py).
# Where the name lives: tests/test_schedule_fused_cpu.py::test_constant_and_header takes every integer of vars(hip) whose name ends
# in _FLAG (or starts with FLAG_) for a bit below SCHEDULE_FUSED_FLAG -- seventeen of them, summing to 131071 -- so a bit above it
# cannot be one more integer of the module's dict without failing that test.  Such bits are kept in this table and served by the
# module's __getattr__ / __dir__ (PEP 562): hip.SAMPLED_FUSED_FLAG, getattr and dir(hip) work as for the others, vars(hip) does not
# list it.  Once that test's census is bounded by its own bit, the entry becomes a plain constant like its neighbours
#
# SAMPLED_LISTED_FLAG (RPF_FLAG_SAMPLED_LISTED of the header) modifies SAMPLED_NBHD_FLAG too: a sampled pass of
# the call on a compiled layout (no FLAG_GENERIC, S + draws <= 3136, not forced wide, no schedule gain other than 1 unless
# SCHEDULE_FUSED_FLAG) runs on the listed builds of the compiled kernels, which copy route 8's member lists from the member pool:
# route 12.  Wide windows (box*box*S > 65535 with FLAG_WIDE_NBHD) included; no mask buffer.  With SAMPLED_FUSED_FLAG as well, option
# "sampled_listed_stride" picks between routes 11 and 12 where both apply.  Every other pass runs as without it.  Refused without
# SAMPLED_NBHD_FLAG.  Its table: tests/test_sampled_listed_cpu.py
#
# GENERIC_QUAD_FLAG (RPF_FLAG_GENERIC_QUAD of the header) modifies FLAG_GENERIC | FLAG_GENERIC_PACKED |
# FLAG_GENERIC_WAVE: the pixels with 832 < N <= 3136 run on the four-wave layout-generic kernels (size classes 1600 and 3136, where
# generic_quad_carve says the layout fits them) and only what lies above stays on the generic filter kernel: route 13 for a pass with
# S <= 3136.  A wide, sampled or member-test pass runs as without it.  fp64 only: refused without all three of those flags and with
# FLAG_FAST_WEIGHTS, FLAG_GENERIC_FAST or FLAG_STREAM_FAST.  Its table: tests/test_generic_quad_cpu.py
_LATER_BITS = {"SAMPLED_FUSED_FLAG": 262144, "SAMPLED_LISTED_FLAG": 524288, "GENERIC_QUAD_FLAG": 1048576}


def __getattr__(name):
    try:
        return _LATER_BITS[name]
    except KeyError:
        raise AttributeError("module %r has no attribute %r" % (__name__, name)) from None


def __dir__():
    return sorted(set(globals()) | set(_LATER_BITS))


# the per-pass activity report (Context.pass_report): every pass of the call leaves one PassReport, reduced on
# the device from its input colours, its output colours (before the spike pass), N, alpha, beta and W_r_c over the filtered rows.
# Changes no result, counter, route or launch count; every filter entry point and filter_pass_debug (entry 0) take it; in
# Context.filter it implies the serial order of FLAG_NO_OVERLAP.  RPF_FLAG_PASS_REPORT of the header; the name stays outside the
# FLAG_* family for SAMPLED_NBHD_FLAG's reason (tests/test_flag_table_cpu.py holds FLAG_* to eleven bits)
PASS_REPORT_FLAG = 32768
REPORT_NCLASS = 9  # RPF_REPORT_NCLASS: N <= 8, 16, 32, 64, 128, 256, 448, 832, and above
FLAG_WIDE_NBHD = 64  # passes with 65535 < box*box*S <= 262144 on the wide layout-generic kernel (route 6); max_nbhd() tells the bound
MAX_NDIM = 40     # the layout-generic kernels take 5 + n_random + n_feat up to this
PLANES_F32, PLANES_F16 = 0, 1

EXPORTS = ["rpf_version", "rpf_status_string", "rpf_create", "rpf_destroy", "rpf_last_error", "rpf_filter",
           "rpf_filter_device", "rpf_colour_from_planes_device", "rpf_reduce_device", "rpf_stage_pixel_stats",
           "rpf_filter_pass_debug", "rpf_query_counters", "rpf_lds_bytes_required", "rpf_check_window_span", "rpf_selftest_udiv", "rpf_feature_images",
           "rpf_host_alloc", "rpf_host_free", "rpf_filter_ex", "rpf_set_option", "rpf_check_option", "rpf_multi_create", "rpf_multi_destroy",
           "rpf_multi_last_error", "rpf_multi_device_count", "rpf_multi_set_option", "rpf_multi_filter",
           "rpf_multi_query_counters", "rpf_query_nbhd", "rpf_query_route", "rpf_film_filter_table", "rpf_filter_film",
           "rpf_film_splat_device", "rpf_film_window", "rpf_multi_halo_plan", "rpf_multi_filter_film", "rpf_layout_kernels",
           "rpf_max_nbhd", "rpf_wide_table", "rpf_set_spike", "rpf_multi_set_spike", "rpf_query_spike", "rpf_multi_query_spike",
           "rpf_spike_clamp_device", "rpf_colour_add_device", "rpf_spike_delta", "rpf_set_sampling", "rpf_multi_set_sampling",
           "rpf_sampling_table", "rpf_sampling_draws", "rpf_set_membership", "rpf_multi_set_membership", "rpf_membership_preset",
           "rpf_set_schedule", "rpf_multi_set_schedule", "rpf_schedule_preset", "rpf_max_draws", "rpf_generic_quad_carve", "rpf_query_pass_report",
           "rpf_query_pass_report_rows", "rpf_multi_query_pass_report", "rpf_pass_report_rows_device", "rpf_pass_report_fold"]

# the film step: pbrt's PixelFilters (include/rpf_hip.h, rpf_film)
PIXFILTER_BOX, PIXFILTER_TRIANGLE, PIXFILTER_GAUSSIAN, PIXFILTER_MITCHELL, PIXFILTER_SINC = range(5)
FILTER_TABLE_WIDTH = 16
# pbrt's default radius per filter (box.cpp:44-45, triangle.cpp:46-47, gaussian.cpp:44-45, mitchell.cpp:57-58, sinc.cpp:54-55)
DEFAULT_RADIUS = {PIXFILTER_BOX: 0.5, PIXFILTER_TRIANGLE: 2.0, PIXFILTER_GAUSSIAN: 2.0, PIXFILTER_MITCHELL: 2.0, PIXFILTER_SINC: 4.0}


class Desc(C.Structure):
    _fields_ = [("W", C.c_int32), ("H", C.c_int32), ("S", C.c_int32), ("row_begin", C.c_int32),
                ("row_end", C.c_int32), ("n_box", C.c_int32), ("box_sizes", C.c_int32 * MAX_BOXES),
                ("beta_map", C.c_int32), ("degenerate_policy", C.c_int32), ("flags", C.c_int32),
                ("eps", C.c_double), ("sigma_seed", C.c_double), ("n_random", C.c_int32), ("n_feat", C.c_int32),
                ("plane_dtype", C.c_int32), ("reserved", C.c_int32)]


def dims(desc):
    """(ndim, nfeat, npair, numpy plane dtype) of a descriptor's sample layout (0 fields = the reference's)"""
    nr, nf = desc.n_random or 2, desc.n_feat or 12
    return 5 + nr + nf, nf, nf * (nr + 2) + 3 * (nr + 2 + nf), (np.float16 if desc.plane_dtype == PLANES_F16 else np.float32)


class Debug(C.Structure):
    _fields_ = [("nbhd_size", C.c_void_p), ("mean", C.c_void_p), ("stddev", C.c_void_p), ("mi", C.c_void_p),
                ("alpha", C.c_void_p), ("beta", C.c_void_p), ("wrc", C.c_void_p), ("bin_hash", C.c_void_p),
                ("member_hash", C.c_void_p)]


class Counters(C.Structure):
    _fields_ = [("samples_filtered", C.c_int64), ("sum_nbhd", C.c_int64), ("nonfinite_pixels", C.c_int64),
                ("max_nbhd", C.c_int32), ("first_bad_pixel", C.c_int32), ("filter_kernel_ms", C.c_float),
                ("stats_kernel_ms", C.c_float), ("device_total_ms", C.c_float), ("h2d_ms", C.c_float),
                ("d2h_ms", C.c_float), ("filter_kernel_launches", C.c_int32), ("options_active", C.c_int32),
                ("redo_pixels", C.c_int32)]


class SpikeStats(C.Structure):
    """rpf_spike_stats: the spike pass of the most recent call (applied = 0 and zeros when FLAG_SPIKE_CLAMP was off)"""
    _fields_ = [("spike_samples", C.c_int64), ("spike_pixels", C.c_int64), ("skipped_pixels", C.c_int64),
                ("energy", C.c_double * 3), ("delta", C.c_double * 3), ("spike_ms", C.c_float), ("applied", C.c_int32)]


class ReportRow(C.Structure):
    """rpf_report_row, 920 bytes: the record of one row of one pass (or, as PassReport.total, the fold of the rows).  Offsets:
    moved2 0 | in2 24 | pix_moved2 48 | pix_in2 72 | alpha_sum 96 | wrc_sum 120 | beta_sum 128 (MAX_NDIM doubles) | sum_nbhd 448 |
    own_only_pixels 456 | class_pixels 464 (REPORT_NCLASS int64) | unchanged_samples 536 | nonfinite_samples 544 |
    nonfinite_pixels 552 | weights_nonfinite 560 | alpha_zero 568 | beta_zero 592 (MAX_NDIM int64) | min_nbhd 912 | max_nbhd 916"""
    _fields_ = [("moved2", C.c_double * 3), ("in2", C.c_double * 3), ("pix_moved2", C.c_double * 3), ("pix_in2", C.c_double * 3),
                ("alpha_sum", C.c_double * 3), ("wrc_sum", C.c_double), ("beta_sum", C.c_double * MAX_NDIM),
                ("sum_nbhd", C.c_int64), ("own_only_pixels", C.c_int64), ("class_pixels", C.c_int64 * REPORT_NCLASS),
                ("unchanged_samples", C.c_int64), ("nonfinite_samples", C.c_int64), ("nonfinite_pixels", C.c_int64),
                ("weights_nonfinite", C.c_int64), ("alpha_zero", C.c_int64 * 3), ("beta_zero", C.c_int64 * MAX_NDIM),
                ("min_nbhd", C.c_int32), ("max_nbhd", C.c_int32)]


class PassReport(C.Structure):
    """rpf_pass_report, 960 bytes: applied 0 | box 4 | draws 8 | route 12 | rows 16 | pixels 24 | samples 32 | total 40.
    applied = 0 and zeros when the most recent call did not fill the entry (PASS_REPORT_FLAG off, or fewer passes)"""
    _fields_ = [("applied", C.c_int32), ("box", C.c_int32), ("draws", C.c_int32), ("route", C.c_int32), ("rows", C.c_int32),
                ("pixels", C.c_int64), ("samples", C.c_int64), ("total", ReportRow)]


def pass_report_fold(rows):
    """rpf_pass_report_fold (no GPU needed): the ReportRow that folds `rows` (a ctypes array or a sequence of ReportRow) in their
    order -- doubles as a serial chain, counts summed, min_nbhd / max_nbhd the minimum / maximum; the one fold Context and
    MultiContext use.  None or no row: RPF_E_BADARG"""
    n = 0 if rows is None else len(rows)
    arr = None
    if n:
        arr = rows if isinstance(rows, C.Array) else (ReportRow * n)(*rows)
    out = ReportRow()
    st = load().rpf_pass_report_fold(arr, n, C.byref(out))
    if st != OK:
        raise RpfError(st, "rpf_pass_report_fold(n_rows=%r): a NULL pointer or a non-positive count" % (n,))
    return out


class Sampling(C.Structure):
    """rpf_sampling: pass p of a call has id pass_id0 + p and draws[p] draws per pixel (0: the pass runs as without
    SAMPLED_NBHD_FLAG); row_origin is the image row of buffer row 0"""
    _fields_ = [("seed", C.c_uint64), ("pass_id0", C.c_int32), ("row_origin", C.c_int32), ("draws", C.c_int32 * MAX_BOXES)]


def make_sampling(seed, draws, pass_id0=0, row_origin=0):
    s = Sampling()
    s.seed, s.pass_id0, s.row_origin = int(seed), int(pass_id0), int(row_origin)
    for i, d in enumerate(list(draws)[:MAX_BOXES]):
        s.draws[i] = int(d)
    return s


class Membership(C.Structure):
    """rpf_membership: feature k < n_feat is rejected iff |f_k - m_k| >= sd_k * mult[k] and |f_k - m_k| > (sd_k > floor[k] ? -inf :
    floor[k]); all MAX_NDIM entries are validated (mult finite and > 0, floor neither NaN nor +inf)"""
    _fields_ = [("mult", C.c_double * MAX_NDIM), ("floor", C.c_double * MAX_NDIM)]


MEMBERSHIP_REFERENCE, MEMBERSHIP_PUBLISHED_19 = 0, 1


def make_membership(mult, floor):
    """a Membership from two sequences (or two scalars, for every feature); entries not given are the reference's 3 and -1"""
    m = Membership()
    for k in range(MAX_NDIM):
        m.mult[k], m.floor[k] = 3.0, -1.0
    mu = [mult] * MAX_NDIM if np.isscalar(mult) else list(mult)
    fl = [floor] * MAX_NDIM if np.isscalar(floor) else list(floor)
    for k, v in enumerate(mu[:MAX_NDIM]):
        m.mult[k] = float(v)
    for k, v in enumerate(fl[:MAX_NDIM]):
        m.floor[k] = float(v)
    return m


def membership_preset(kind, n_feat=NFEAT):
    """rpf_membership_preset (no GPU needed): kind MEMBERSHIP_REFERENCE -- multiples 3, floors -1 -- or MEMBERSHIP_PUBLISHED_19 --
    multiples 3, 30 on the world positions (features 3..5 and 9..11), floors 0.1; n_feat must be 12.  The constants of the latter
    are from memory of the paper, and a floor on a world position depends on the scene's scale: set those for the scene"""
    m = Membership()
    st = load().rpf_membership_preset(int(kind), int(n_feat), C.byref(m))
    if st != OK:
        raise RpfError(st, "rpf_membership_preset(kind=%r, n_feat=%r): an unknown kind, n_feat outside [1, 40], or kind 1 with n_feat != 12" % (kind, n_feat))
    return m


class Schedule(C.Structure):
    """rpf_schedule: pass p of a call reads entry pass0 + p; all MAX_BOXES entries are validated (seed finite and > 0, gains finite
    and >= 0, pass0 in [0, MAX_BOXES))"""
    _fields_ = [("pass0", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_double * MAX_BOXES),
                ("gain_c", C.c_double * MAX_BOXES), ("gain_f", C.c_double * MAX_BOXES)]


SCHEDULE_REFERENCE, SCHEDULE_PUBLISHED = 0, 1


def make_schedule(seed, gain_c, gain_f, pass0=0):
    """a Schedule from three sequences (or scalars, for every entry); entries not given are the reference's 0.002, 1, 1"""
    sc = Schedule()
    sc.pass0, sc.reserved = int(pass0), 0
    for e in range(MAX_BOXES):
        sc.seed[e], sc.gain_c[e], sc.gain_f[e] = 0.002, 1.0, 1.0
    for dst, src in ((sc.seed, seed), (sc.gain_c, gain_c), (sc.gain_f, gain_f)):
        vals = [src] * MAX_BOXES if np.isscalar(src) else list(src)
        for e, v in enumerate(vals[:MAX_BOXES]):
            dst[e] = float(v)
    return sc


def schedule_preset(kind, S):
    """rpf_schedule_preset (no GPU needed): kind SCHEDULE_REFERENCE -- seeds 0.002, gains 1 -- or SCHEDULE_PUBLISHED -- seed[t] =
    sqrt(8 v_t / S) with v_0 = 0.02, v_t = 0.002 otherwise, gain_c[t] = 2 (1 + 0.1 t), gain_f[t] = 1 + 0.1 t.  The constants of the
    latter are from memory of the paper; nothing in the library depends on them"""
    sc = Schedule()
    st = load().rpf_schedule_preset(int(kind), int(S), C.byref(sc))
    if st != OK:
        raise RpfError(st, "rpf_schedule_preset(kind=%r, S=%r): an unknown kind or S <= 0" % (kind, S))
    return sc


def sampling_table(box):
    """rpf_sampling_table (no GPU needed): uint32 [box - 1], the Gaussian thresholds of an odd box"""
    out = np.zeros(max(int(box) - 1, 1), np.uint32)
    st = load().rpf_sampling_table(int(box), _p(out))
    if st != OK:
        raise RpfError(st, "rpf_sampling_table(box=%r): an even box, or a box outside [1, 511]" % (box,))
    return out[:int(box) - 1]


def sampling_draws(cfg, pass_index, box, W, H, S, x, y):
    """rpf_sampling_draws (no GPU needed): int32 array, the distinct surviving visiting-order indices of buffer pixel (x, y) in
    pass `pass_index` of cfg, ascending, before the 3-sigma test"""
    out = np.zeros(max(int(cfg.draws[pass_index]) if 0 <= pass_index < MAX_BOXES else 0, 1), np.int32)
    n = C.c_int32(0)
    st = load().rpf_sampling_draws(C.byref(cfg), int(pass_index), int(box), int(W), int(H), int(S), int(x), int(y), _p(out), C.byref(n))
    if st != OK:
        raise RpfError(st, "rpf_sampling_draws(pass=%r, box=%r, W=%r, H=%r, S=%r, x=%r, y=%r)" % (pass_index, box, W, H, S, x, y))
    return out[:n.value].copy()


def spike_delta(row_sums, n_samples):
    """rpf_spike_delta (no GPU needed): (energy[3], delta[3]) -- the serial fold of row_sums [n_rows][3] in row order and its
    quotient by n_samples = rows * W * S; the one fold Context and MultiContext use"""
    rs = np.ascontiguousarray(row_sums, np.float64)
    assert rs.ndim == 2 and rs.shape[1] == 3, rs.shape
    e, d = np.empty(3), np.empty(3)
    st = load().rpf_spike_delta(_p(rs), rs.shape[0], int(n_samples), _p(e), _p(d))
    if st != OK:
        raise RpfError(st, "rpf_spike_delta(n_rows=%r, n_samples=%r): a non-positive count" % (rs.shape[0], n_samples))
    return e, d


class Film(C.Structure):
    _fields_ = [("sample_x0", C.c_int32), ("sample_y0", C.c_int32), ("px0", C.c_int32), ("py0", C.c_int32),
                ("px1", C.c_int32), ("py1", C.c_int32), ("radius_x", C.c_float), ("radius_y", C.c_float),
                ("max_sample_luminance", C.c_float), ("scale", C.c_float),
                ("table", C.c_float * (FILTER_TABLE_WIDTH * FILTER_TABLE_WIDTH))]


def film_table(kind, radius=None, p0=None, p1=None):
    """pbrt's filter table (rpf_film_filter_table): float32 [16][16], [y][x].  radius: float or (rx, ry), None = pbrt's
    default for the filter; p0 / p1: gaussian alpha | mitchell B, C | sinc tau, None = pbrt's default"""
    rx, ry = _radii(kind, radius)
    out = np.empty((FILTER_TABLE_WIDTH, FILTER_TABLE_WIDTH), np.float32)
    nan = float("nan")
    st = load().rpf_film_filter_table(int(kind), rx, ry, nan if p0 is None else p0, nan if p1 is None else p1, _p(out))
    if st != OK:
        raise RpfError(st, "rpf_film_filter_table(kind=%r, radius=(%r, %r))" % (kind, rx, ry))
    return out


def _radii(kind, radius):
    if radius is None:
        radius = DEFAULT_RADIUS.get(int(kind), 1.0)
    rx, ry = (radius, radius) if np.isscalar(radius) else radius
    return float(rx), float(ry)


def film_window(desc, film):
    """(half_x, half_y) of the film step's gather for the buffer of `desc` as the sample film (rpf_film_window; no GPU
    needed): half_y is the number of rows of each neighbour a row slab must hold for the film step"""
    hx, hy = C.c_int32(0), C.c_int32(0)
    st = load().rpf_film_window(C.byref(desc), C.byref(film), C.byref(hx), C.byref(hy))
    if st != OK:
        raise RpfError(st, "rpf_film_window: the film step refuses this descriptor / film (see rpf_filter_film)")
    return hx.value, hy.value


def layout_kernels(desc):
    """rpf_layout_kernels (no GPU needed): (status, generic) for the layout and flags of `desc` -- (OK, 0) the compiled fused
    kernels, (OK, 1) the layout-generic kernels (FLAG_GENERIC; FLAG_GENERIC_FAST does not change the answer),
    (E_UNSUPPORTED, None) where the filter entry points refuse it -- FLAG_GENERIC_FAST without FLAG_GENERIC | FLAG_GENERIC_PACKED,
    with FLAG_FAST_WEIGHTS or with FLAG_WIDE_NBHD, and FLAG_STREAM_FAST without either of FLAG_GENERIC and FLAG_WIDE_NBHD, among them
    (where FLAG_STREAM_FAST is accepted the answer is that of the same flags without it); desc None: (E_BADARG, None)"""
    g = C.c_int32(-1)
    st = load().rpf_layout_kernels(None if desc is None else C.byref(desc), C.byref(g))
    return st, (g.value if st == OK else None)


def max_nbhd(desc):
    """rpf_max_nbhd (no GPU needed): (status, nmax) -- the largest box*box*S a pass may have under the flags of `desc`: (OK, 65535),
    or (OK, 262144) with FLAG_WIDE_NBHD; desc None: (E_BADARG, None)"""
    n = C.c_int32(-1)
    st = load().rpf_max_nbhd(None if desc is None else C.byref(desc), C.byref(n))
    return st, (n.value if st == OK else None)


def check_option(name, value):
    """rpf_check_option (no GPU needed): OK when Context.set_option would take (name, value), else E_BADARG"""
    return load().rpf_check_option(name.encode(), int(value))


def max_draws(desc):
    """rpf_max_draws (no GPU needed): (status, dmax) -- the most draws a sampled pass may have under S and the flags of `desc`:
    (OK, max(0, 832 - S)), or (OK, max(0, SAMPLED_MAX - S)) with SAMPLED_REST_FLAG; desc None or S <= 0: (E_BADARG, None)"""
    n = C.c_int32(-1)
    st = load().rpf_max_draws(None if desc is None else C.byref(desc), C.byref(n))
    return st, (n.value if st == OK else None)


def generic_quad_carve(desc, capacity):
    """rpf_generic_quad_carve (no GPU needed): (status, workgroups_per_cu, lds_bytes) -- what the layout of `desc` gets from
    GENERIC_QUAD_FLAG at the size class `capacity` (1600 or 3136): OK when the four-wave kernel's LDS carve-up fits, E_UNSUPPORTED
    when it does not (route 13 leaves that class to the generic filter kernel), E_BADARG for any other capacity or desc None"""
    wg, lds = C.c_int32(-1), C.c_int64(-1)
    st = load().rpf_generic_quad_carve(None if desc is None else C.byref(desc), int(capacity), C.byref(wg), C.byref(lds))
    return st, (wg.value if st == OK else None), (lds.value if st == OK else None)


def wide_table(nmax):
    """rpf_wide_table (no GPU needed): uint64 [nmax + 1], round(k ln k * 2^41) -- the table the wide kernel forms MI from"""
    out = np.empty(nmax + 1, np.uint64)
    st = load().rpf_wide_table(int(nmax), _p(out))
    if st != OK:
        raise RpfError(st, "rpf_wide_table(nmax=%r): nmax outside [0, 262144]" % (nmax,))
    return out


def halo_plan(H, n_slabs, depth):
    """rpf_multi_halo_plan (no GPU needed): (slabs, copies).  slabs[g] = (a, b, ht, hb): owned image rows [a, b) and the
    halo rows held, what slabs.slab_for gives; copies = [(source slab, source buffer row, destination slab, destination
    buffer row, rows)]: a refresh of every halo row from the neighbour's owned boundary rows"""
    n = max(int(n_slabs), 1)
    sl, cp, nc = (C.c_int32 * (4 * n))(), (C.c_int32 * (10 * n))(), C.c_int32(0)
    st = load().rpf_multi_halo_plan(H, n_slabs, depth, sl, cp, C.byref(nc))
    if st != OK:
        raise RpfError(st, "rpf_multi_halo_plan(H=%r, n_slabs=%r, depth=%r): bad argument, or a slab owns fewer rows than "
                           "the depth" % (H, n_slabs, depth))
    return ([tuple(sl[4 * g:4 * g + 4]) for g in range(n_slabs)], [tuple(cp[5 * i:5 * i + 5]) for i in range(nc.value)])


def make_film(pixel_bounds, radius, table, sample_origin=None, max_sample_luminance=float("inf"), scale=1.0):
    """rpf_film for croppedPixelBounds ((px0, py0), (px1, py1)) and a filter of `radius` (float or (rx, ry)) with its 16x16
    `table`.  sample_origin None = Film::GetSampleBounds().pMin: floor(p0 + 0.5 - r) per axis (film.cpp:80-86)."""
    (px0, py0), (px1, py1) = pixel_bounds
    rx, ry = _radii(None, radius)
    if sample_origin is None:
        sample_origin = (int(np.floor(np.float32(px0) + np.float32(0.5) - np.float32(rx))),
                         int(np.floor(np.float32(py0) + np.float32(0.5) - np.float32(ry))))
    f = Film()
    f.sample_x0, f.sample_y0 = sample_origin
    f.px0, f.py0, f.px1, f.py1 = px0, py0, px1, py1
    f.radius_x, f.radius_y = rx, ry
    f.max_sample_luminance, f.scale = max_sample_luminance, scale
    C.memmove(f.table, np.ascontiguousarray(table, np.float32).ctypes.data, C.sizeof(f.table))
    return f


class RpfError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("%s: %s" % (status_string(status), message))
        self.status = status


_lib = None


def load():
    """dlopen librpf_hip.so; raises OSError when it has not been built (``__graft_entry__.build()``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("librpf_hip.so is missing (%s): run `python -c 'import __graft_entry__ as g; g.build()'`. "
                          "There is no CPU fallback." % LIB_PATH)
        try:
            # PyTorch wheels bundle their own HIP runtime; when torch is used in the same process (HBM tensors,
            # streams, torch.distributed) it must be the first to load libamdhip64 so that both sides share ONE
            # runtime -- loading ours first leaves torch unable to see the GPU.
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.rpf_version.restype = C.c_char_p
        L.rpf_status_string.restype = C.c_char_p
        L.rpf_status_string.argtypes = [C.c_int32]
        L.rpf_create.argtypes = [C.POINTER(C.c_void_p), C.c_int32]
        L.rpf_destroy.argtypes = [C.c_void_p]
        L.rpf_destroy.restype = None
        L.rpf_last_error.restype = C.c_char_p
        L.rpf_last_error.argtypes = [C.c_void_p]
        L.rpf_filter.argtypes = [C.c_void_p, C.POINTER(Desc)] + [C.c_void_p] * 4
        L.rpf_filter_ex.argtypes = [C.c_void_p, C.POINTER(Desc)] + [C.c_void_p] * 6
        L.rpf_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        if hasattr(L, "rpf_check_option"):  # (absent from a build of before the symbol, loaded through RPF_HIP_LIB)
            L.rpf_check_option.argtypes = [C.c_char_p, C.c_int64]
        L.rpf_filter_device.argtypes = [C.c_void_p, C.POINTER(Desc)] + [C.c_void_p] * 3
        L.rpf_colour_from_planes_device.argtypes = [C.c_void_p, C.POINTER(Desc)] + [C.c_void_p] * 3
        L.rpf_reduce_device.argtypes = [C.c_void_p, C.POINTER(Desc)] + [C.c_void_p] * 5
        L.rpf_stage_pixel_stats.argtypes = [C.c_void_p, C.POINTER(Desc)] + [C.c_void_p] * 3
        L.rpf_filter_pass_debug.argtypes = [C.c_void_p, C.POINTER(Desc), C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.POINTER(Debug)]
        L.rpf_query_counters.argtypes = [C.c_void_p, C.POINTER(Counters)]
        L.rpf_query_nbhd.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        L.rpf_query_route.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.rpf_selftest_udiv.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int32, C.POINTER(C.c_uint64)]
        L.rpf_feature_images.argtypes = [C.c_void_p, C.POINTER(Desc), C.c_void_p, C.c_void_p]
        L.rpf_lds_bytes_required.restype = C.c_int64
        L.rpf_lds_bytes_required.argtypes = [C.c_int32, C.c_int32]
        if hasattr(L, "rpf_check_window_span"):  # (a build from before the symbol, loaded through RPF_HIP_LIB to be measured side by side)
            L.rpf_check_window_span.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        L.rpf_multi_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32]
        L.rpf_multi_destroy.argtypes = [C.c_void_p]
        L.rpf_multi_destroy.restype = None
        L.rpf_multi_last_error.restype = C.c_char_p
        L.rpf_multi_last_error.argtypes = [C.c_void_p]
        L.rpf_multi_device_count.argtypes = [C.c_void_p]
        L.rpf_multi_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.rpf_multi_filter.argtypes = [C.c_void_p, C.POINTER(Desc)] + [C.c_void_p] * 4
        L.rpf_multi_query_counters.argtypes = [C.c_void_p, C.POINTER(Counters)]
        L.rpf_film_filter_table.argtypes = [C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]
        L.rpf_filter_film.argtypes = [C.c_void_p, C.POINTER(Desc), C.POINTER(Film)] + [C.c_void_p] * 6
        L.rpf_film_splat_device.argtypes = [C.c_void_p, C.POINTER(Desc), C.POINTER(Film)] + [C.c_void_p] * 7
        if hasattr(L, "rpf_multi_filter_film"):  # (absent from a build of before the film step on slabs, loaded through RPF_HIP_LIB)
            L.rpf_film_window.argtypes = [C.POINTER(Desc), C.POINTER(Film), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
            L.rpf_multi_halo_plan.argtypes = [C.c_int32] * 3 + [C.POINTER(C.c_int32)] * 3
            L.rpf_multi_filter_film.argtypes = [C.c_void_p, C.POINTER(Desc), C.POINTER(Film)] + [C.c_void_p] * 6
        if hasattr(L, "rpf_layout_kernels"):  # (absent from a build of before the generic route, loaded through RPF_HIP_LIB)
            L.rpf_layout_kernels.argtypes = [C.POINTER(Desc), C.POINTER(C.c_int32)]
        if hasattr(L, "rpf_max_nbhd"):  # (absent from a build of before the wide route, loaded through RPF_HIP_LIB)
            L.rpf_max_nbhd.argtypes = [C.POINTER(Desc), C.POINTER(C.c_int32)]
            L.rpf_wide_table.argtypes = [C.c_int32, C.c_void_p]
        if hasattr(L, "rpf_set_spike"):  # (absent from a build of before the spike pass, loaded through RPF_HIP_LIB)
            L.rpf_set_spike.argtypes = [C.c_void_p, C.c_double, C.c_int32]
            L.rpf_multi_set_spike.argtypes = [C.c_void_p, C.c_double, C.c_int32]
            L.rpf_query_spike.argtypes = [C.c_void_p, C.POINTER(SpikeStats)]
            L.rpf_multi_query_spike.argtypes = [C.c_void_p, C.POINTER(SpikeStats)]
            L.rpf_spike_clamp_device.argtypes = [C.c_void_p, C.POINTER(Desc), C.c_void_p, C.c_double, C.c_void_p,
                                                 C.POINTER(SpikeStats), C.c_void_p]
            L.rpf_colour_add_device.argtypes = [C.c_void_p, C.POINTER(Desc), C.c_void_p, C.c_void_p, C.c_void_p]
            L.rpf_spike_delta.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        if hasattr(L, "rpf_set_sampling"):  # (absent from a build of before sampled neighbourhoods, loaded through RPF_HIP_LIB)
            L.rpf_set_sampling.argtypes = [C.c_void_p, C.POINTER(Sampling)]
            L.rpf_multi_set_sampling.argtypes = [C.c_void_p, C.POINTER(Sampling)]
            L.rpf_sampling_table.argtypes = [C.c_int32, C.c_void_p]
            L.rpf_sampling_draws.argtypes = [C.POINTER(Sampling)] + [C.c_int32] * 7 + [C.c_void_p, C.POINTER(C.c_int32)]
        if hasattr(L, "rpf_set_membership"):  # (absent from a build of before the membership test, loaded through RPF_HIP_LIB)
            L.rpf_set_membership.argtypes = [C.c_void_p, C.POINTER(Membership)]
            L.rpf_multi_set_membership.argtypes = [C.c_void_p, C.POINTER(Membership)]
            L.rpf_membership_preset.argtypes = [C.c_int32, C.c_int32, C.POINTER(Membership)]
        if hasattr(L, "rpf_set_schedule"):  # (absent from a build of before the schedule, loaded through RPF_HIP_LIB)
            L.rpf_set_schedule.argtypes = [C.c_void_p, C.POINTER(Schedule)]
            L.rpf_multi_set_schedule.argtypes = [C.c_void_p, C.POINTER(Schedule)]
            L.rpf_schedule_preset.argtypes = [C.c_int32, C.c_int32, C.POINTER(Schedule)]
        if hasattr(L, "rpf_max_draws"):  # (absent from a build of before the listed rest launch, loaded through RPF_HIP_LIB)
            L.rpf_max_draws.argtypes = [C.POINTER(Desc), C.POINTER(C.c_int32)]
        if hasattr(L, "rpf_generic_quad_carve"):  # (absent from a build of before the four-wave generic kernels, loaded through RPF_HIP_LIB)
            L.rpf_generic_quad_carve.argtypes = [C.POINTER(Desc), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
        if hasattr(L, "rpf_query_pass_report"):  # (absent from a build of before the pass report, loaded through RPF_HIP_LIB)
            L.rpf_query_pass_report.argtypes = [C.c_void_p, C.c_int32, C.POINTER(PassReport)]
            L.rpf_query_pass_report_rows.argtypes = [C.c_void_p, C.c_int32, C.POINTER(ReportRow), C.c_int64]
            L.rpf_multi_query_pass_report.argtypes = [C.c_void_p, C.c_int32, C.POINTER(PassReport)]
            L.rpf_pass_report_rows_device.argtypes = [C.c_void_p, C.POINTER(Desc)] + [C.c_void_p] * 6 + [C.POINTER(ReportRow), C.c_void_p]
            L.rpf_pass_report_fold.argtypes = [C.POINTER(ReportRow), C.c_int64, C.POINTER(ReportRow)]
        L.rpf_host_alloc.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
        L.rpf_host_free.argtypes = [C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def status_string(st):
    return load().rpf_status_string(int(st)).decode()


def make_desc(W, H, S, boxes=(7,), row_begin=0, row_end=None, beta_map=BETA_REF_GCC11_O3, policy=DEGEN_REF_ABORT,
              eps=1e-10, sigma_seed=0.002, flags=0, n_random=0, n_feat=0, plane_dtype=PLANES_F32):
    d = Desc()
    d.W, d.H, d.S = W, H, S
    d.row_begin, d.row_end = row_begin, (H if row_end is None else row_end)
    d.n_box = len(boxes)
    for i, b in enumerate(boxes[:MAX_BOXES]):
        d.box_sizes[i] = b
    d.beta_map, d.degenerate_policy, d.flags = beta_map, policy, flags
    d.eps, d.sigma_seed = eps, sigma_seed
    d.n_random, d.n_feat, d.plane_dtype = n_random, n_feat, plane_dtype
    return d


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Context:
    """One rpf_ctx (one HIP device).  Mirrors how RPFIntegrator::Render drives ApplyRPFFilter."""

    def __init__(self, device=0):
        self._L = load()
        h = C.c_void_p()
        st = self._L.rpf_create(C.byref(h), device)
        self._h = h
        if st != OK:
            msg = self._L.rpf_last_error(h).decode() if h else "no HIP device"
            if h:
                self._L.rpf_destroy(h)
                self._h = None
            raise RpfError(st, msg)

    def close(self):
        if getattr(self, "_h", None):
            self._L.rpf_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, st, allow=()):
        if st != OK and st not in allow:
            raise RpfError(st, self._L.rpf_last_error(self._h).decode())
        return st

    def set_option(self, name, value):
        """per-context tuning / diagnostic override (rpf_set_option); see include/rpf_hip.h for the names"""
        self._check(self._L.rpf_set_option(self._h, name.encode(), int(value)))

    def counters(self):
        c = Counters()
        self._check(self._L.rpf_query_counters(self._h, C.byref(c)))
        return c

    def nbhd(self, W, H):
        """neighbourhood size of every pixel as the last pass of the most recent call left it (rpf_query_nbhd)"""
        out = np.empty((H, W), np.int32)
        self._check(self._L.rpf_query_nbhd(self._h, _p(out), W * H))
        return out

    def route(self):
        """kernel route of the last pass: 0 fused, 1 count first, 2 size-binned, 3 the layout-generic kernels
        (FLAG_GENERIC), 4 the same with small neighbourhoods packed (FLAG_GENERIC_PACKED), 5 the same with
        64 < N <= 832 on the one-wave generic kernels (FLAG_GENERIC_WAVE; 3 for a pass with S > 832), 6 the wide kernel
        (FLAG_WIDE_NBHD on a pass with box*box*S > 65535), 7 such a pass dealt by size class (FLAG_WIDE_CLASSES), 8 a sampled
        pass (SAMPLED_NBHD_FLAG with draws > 0), 9 a full-box pass under MEMBER_TEST_FLAG, 10 such a pass on the compiled kernels (MEMBER_FUSED_FLAG), 11 a sampled pass on the compiled kernels (SAMPLED_FUSED_FLAG), 12 a sampled pass on their listed builds (SAMPLED_LISTED_FLAG), 13 route 5 with 832 < N <= 3136 on the four-wave generic kernels (GENERIC_QUAD_FLAG; a pass with S <= 3136); -1 before any pass.  FLAG_GENERIC_FAST and FLAG_STREAM_FAST change no route
        (rpf_query_route)"""
        r = C.c_int32(-1)
        self._check(self._L.rpf_query_route(self._h, C.byref(r)))
        return r.value

    # ---- the spike pass (FLAG_SPIKE_CLAMP) --------------------------------------------------------------
    def set_spike(self, threshold=1.0, preserve_energy=True):
        """rpf_set_spike: threshold in standard deviations (finite, > 0), preserve_energy False / True (0 / 1)"""
        self._check(self._L.rpf_set_spike(self._h, float(threshold), int(preserve_energy)))

    def spike_stats(self):
        """rpf_query_spike: SpikeStats of the most recent call"""
        s = SpikeStats()
        self._check(self._L.rpf_query_spike(self._h, C.byref(s)))
        return s

    # ---- sampled neighbourhoods (SAMPLED_NBHD_FLAG) ---------------------------------------------------------
    def set_sampling(self, cfg):
        """rpf_set_sampling: cfg a Sampling (make_sampling), or None -> RPF_E_BADARG as the ABI answers a NULL pointer"""
        self._check(self._L.rpf_set_sampling(self._h, None if cfg is None else C.byref(cfg)))

    # ---- the membership test (MEMBER_TEST_FLAG) ---------------------------------------------------------------
    def set_membership(self, cfg):
        """rpf_set_membership: cfg a Membership (make_membership / membership_preset), or None -> RPF_E_BADARG"""
        self._check(self._L.rpf_set_membership(self._h, None if cfg is None else C.byref(cfg)))

    # ---- the per-pass schedule (SCHEDULE_FLAG) ----------------------------------------------------------------
    def set_schedule(self, cfg):
        """rpf_set_schedule: cfg a Schedule (make_schedule / schedule_preset), or None -> RPF_E_BADARG"""
        self._check(self._L.rpf_set_schedule(self._h, None if cfg is None else C.byref(cfg)))

    # ---- the per-pass activity report (PASS_REPORT_FLAG) ------------------------------------------------------
    def pass_report(self, pass_index):
        """rpf_query_pass_report: the PassReport of pass `pass_index` of the most recent call (applied = 0: not filled)"""
        r = PassReport()
        self._check(self._L.rpf_query_pass_report(self._h, int(pass_index), C.byref(r)))
        return r

    def pass_report_rows(self, pass_index, n_rows=None):
        """rpf_query_pass_report_rows: the row records of that pass as a list of ReportRow, in row order; n_rows None =
        the report's own row count (what the ABI requires)"""
        n = self.pass_report(pass_index).rows if n_rows is None else int(n_rows)
        rows = (ReportRow * max(n, 1))()
        self._check(self._L.rpf_query_pass_report_rows(self._h, int(pass_index), rows, n))
        return list(rows[:max(n, 0)])

    def pass_report_rows_device(self, desc, d_col_in, d_col_out, d_nbhd, d_alpha=None, d_beta=None, d_wrc=None, stream=None):
        """rpf_pass_report_rows_device: the row records of rows [row_begin, row_end) of desc from device buffers (raw pointers;
        the three weight planes may be None: their fields are then zero); returns a list of ReportRow"""
        n = max(desc.row_end - desc.row_begin, 0)
        rows = (ReportRow * max(n, 1))()
        self._check(self._L.rpf_pass_report_rows_device(self._h, C.byref(desc), d_col_in, d_col_out, d_nbhd, d_alpha, d_beta, d_wrc,
                                                        rows, stream))
        return list(rows[:n])

    def spike_clamp_device(self, desc, d_colour, threshold=1.0, stream=None):
        """rpf_spike_clamp_device: the clamp half on rows [row_begin, row_end) of device colours (raw pointer, 3 fp64 planes);
        returns (row_sums float64 [rows][3] on the host, SpikeStats of these rows)"""
        rows = np.empty((max(desc.row_end - desc.row_begin, 0), 3))
        s = SpikeStats()
        self._check(self._L.rpf_spike_clamp_device(self._h, C.byref(desc), d_colour, float(threshold), _p(rows), C.byref(s), stream))
        return rows, s

    def colour_add_device(self, desc, d_colour, delta, stream=None):
        """rpf_colour_add_device: c += delta[k] on rows [row_begin, row_end) of device colours; delta: three host doubles"""
        dl = np.ascontiguousarray(delta, np.float64)
        assert dl.shape == (3,), dl.shape
        self._check(self._L.rpf_colour_add_device(self._h, C.byref(desc), d_colour, _p(dl), stream))

    # ---- host-buffer entry points ------------------------------------------------------------------
    def host_empty(self, shape, dtype=np.float32):
        """numpy array in page-locked host memory (rpf_host_alloc); released when the last view of it is collected."""
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        ptr = C.c_void_p()
        self._check(self._L.rpf_host_alloc(self._h, n, C.byref(ptr)))
        buf = (C.c_char * max(n, 1)).from_address(ptr.value)
        weakref.finalize(buf, self._L.rpf_host_free, None, ptr.value)  # released when the last view dies
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def filter(self, planes, desc, ray_weight=None, want_samples=True, want_pixels=True, allow_nonfinite=False,
               out_samples=None, out_pixels=None, colour64_in=None, want_colour64=False):
        nd, _, _, pdt = dims(desc)
        planes = np.ascontiguousarray(planes, pdt)
        assert planes.shape == (nd, desc.H, desc.W, desc.S), planes.shape
        rw = None if ray_weight is None else np.ascontiguousarray(ray_weight, np.float32)
        srgb = out_samples if out_samples is not None else (
            np.empty((3, desc.H, desc.W, desc.S), np.float32) if want_samples else None)
        prgb = out_pixels if out_pixels is not None else (np.empty((desc.H, desc.W, 3), np.float32) if want_pixels else None)
        if colour64_in is not None or want_colour64:
            cin = None if colour64_in is None else np.ascontiguousarray(colour64_in, np.float64)
            c64 = np.empty((3, desc.H, desc.W, desc.S)) if want_colour64 else None
            st = self._L.rpf_filter_ex(self._h, C.byref(desc), _p(planes), _p(cin), _p(rw), _p(srgb), _p(prgb), _p(c64))
            self._check(st, allow=(E_NONFINITE,) if allow_nonfinite else ())
            return srgb, prgb, st, c64
        st = self._L.rpf_filter(self._h, C.byref(desc), _p(planes), _p(rw), _p(srgb), _p(prgb))
        self._check(st, allow=(E_NONFINITE,) if allow_nonfinite else ())
        return srgb, prgb, st

    def filter_film(self, planes, desc, film, ray_weight=None, allow_nonfinite=False):
        """rpf_filter_film: the passes of desc, then pbrt's film step with `film` (make_film).  Returns (sample_rgb
        [3,H,W,S], tile_rgb [ny,nx,3] = contribSum, tile_weight [ny,nx] = filterWeightSum, image_rgb [ny,nx,3] =
        WriteImage's pixel values), nx, ny = the extent of film's pixel bounds."""
        nd, _, _, pdt = dims(desc)
        planes = np.ascontiguousarray(planes, pdt)
        assert planes.shape == (nd, desc.H, desc.W, desc.S), planes.shape
        rw = None if ray_weight is None else np.ascontiguousarray(ray_weight, np.float32)
        nx, ny = max(film.px1 - film.px0, 0), max(film.py1 - film.py0, 0)
        srgb = np.empty((3, desc.H, desc.W, desc.S), np.float32)
        tile, w, img = np.empty((ny, nx, 3), np.float32), np.empty((ny, nx), np.float32), np.empty((ny, nx, 3), np.float32)
        st = self._L.rpf_filter_film(self._h, C.byref(desc), C.byref(film), _p(planes), _p(rw), _p(srgb), _p(tile), _p(w),
                                     _p(img))
        self._check(st, allow=(E_NONFINITE,) if allow_nonfinite else ())
        return srgb, tile, w, img

    def pixel_stats(self, planes, desc):
        _, nf, _, pdt = dims(desc)
        planes = np.ascontiguousarray(planes, pdt)
        m = np.empty((desc.H, desc.W, nf))
        s = np.empty((desc.H, desc.W, nf))
        self._check(self._L.rpf_stage_pixel_stats(self._h, C.byref(desc), _p(planes), _p(m), _p(s)))
        return m, s

    def filter_pass_debug(self, planes, desc, box=7, colour_in=None, debug=True, allow_nonfinite=False):
        nd, nf, npair, pdt = dims(desc)
        planes = np.ascontiguousarray(planes, pdt)
        assert planes.shape == (nd, desc.H, desc.W, desc.S), planes.shape
        H, W, S = desc.H, desc.W, desc.S
        cin = None if colour_in is None else np.ascontiguousarray(colour_in, np.float64)
        out = np.empty((3, H, W, S))
        d, dbg = {}, None
        if debug:
            d = dict(nbhd_size=np.zeros((H, W), np.int32), mean=np.zeros((H, W, nd)), stddev=np.zeros((H, W, nd)),
                     mi=np.zeros((H, W, npair)), alpha=np.zeros((H, W, 3)), beta=np.zeros((H, W, nf)),
                     wrc=np.zeros((H, W)), bin_hash=np.zeros((H, W, nd), np.uint32),
                     member_hash=np.zeros((H, W), np.uint32))
            dbg = Debug(*[_p(d[k]) for k, _ in Debug._fields_])
        st = self._L.rpf_filter_pass_debug(self._h, C.byref(desc), box, _p(planes), _p(cin), _p(out),
                                           C.byref(dbg) if dbg is not None else None)
        self._check(st, allow=(E_NONFINITE,) if allow_nonfinite else ())
        c = self.counters()
        d.update(colour=out, status=st, nonfinite_pixels=c.nonfinite_pixels, first_bad_pixel=c.first_bad_pixel,
                 sum_nbhd=c.sum_nbhd, max_nbhd=c.max_nbhd, filter_kernel_ms=c.filter_kernel_ms)
        return d

    def feature_images(self, planes, desc):
        planes = np.ascontiguousarray(planes, np.float32)
        out = np.empty((6, desc.H, desc.W, 3))
        self._check(self._L.rpf_feature_images(self._h, C.byref(desc), _p(planes), _p(out)))
        return out

    def selftest_udiv(self, n, seed=1, mode=0):
        m = C.c_uint64(0)
        self._check(self._L.rpf_selftest_udiv(self._h, n, seed, mode, C.byref(m)))
        return m.value

    # ---- device-resident entry points (raw device pointers) -----------------------------------------
    def colour_from_planes_device(self, desc, d_planes, d_colour, stream=None):
        self._check(self._L.rpf_colour_from_planes_device(self._h, C.byref(desc), d_planes, d_colour, stream))

    def filter_device(self, desc, d_planes, d_colour, stream=None, allow_nonfinite=False):
        st = self._L.rpf_filter_device(self._h, C.byref(desc), d_planes, d_colour, stream)
        return self._check(st, allow=(E_NONFINITE,) if allow_nonfinite else ())

    def reduce_device(self, desc, d_colour, d_ray_weight, d_sample_rgb, d_pixel_rgb, stream=None):
        self._check(self._L.rpf_reduce_device(self._h, C.byref(desc), d_colour, d_ray_weight, d_sample_rgb,
                                              d_pixel_rgb, stream))

    def film_splat_device(self, desc, film, d_planes, d_colour, d_ray_weight, d_tile_rgb, d_tile_weight, d_image_rgb,
                          stream=None):
        """rpf_film_splat_device: the film step alone on device buffers (raw pointers; any output may be None)"""
        self._check(self._L.rpf_film_splat_device(self._h, C.byref(desc), C.byref(film), d_planes, d_colour, d_ray_weight,
                                                  d_tile_rgb, d_tile_weight, d_image_rgb, stream))


class MultiContext:
    """rpf_multi: one caller, one row slab per entry of ``devices`` (None = every visible GPU; an ordinal may repeat)"""

    def __init__(self, devices=None):
        self._L = load()
        h = C.c_void_p()
        arr = None if devices is None else (C.c_int32 * len(devices))(*devices)
        st = self._L.rpf_multi_create(C.byref(h), arr, 0 if devices is None else len(devices))
        self._h = h
        if st != OK:
            msg = self._L.rpf_multi_last_error(h).decode() if h else "no HIP device"
            if h:
                self._L.rpf_multi_destroy(h)
                self._h = None
            raise RpfError(st, msg)

    def close(self):
        if getattr(self, "_h", None):
            self._L.rpf_multi_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def device_count(self):
        return self._L.rpf_multi_device_count(self._h)

    def counters(self):
        c = Counters()
        self._L.rpf_multi_query_counters(self._h, C.byref(c))
        return c

    def set_spike(self, threshold=1.0, preserve_energy=True):
        """rpf_multi_set_spike: the spike pass's parameters for every slab (Context.set_spike)"""
        st = self._L.rpf_multi_set_spike(self._h, float(threshold), int(preserve_energy))
        if st != OK:
            raise RpfError(st, self._L.rpf_multi_last_error(self._h).decode())

    def set_sampling(self, cfg):
        """rpf_multi_set_sampling: the configuration of every slab (each adds its first image row to cfg.row_origin)"""
        st = self._L.rpf_multi_set_sampling(self._h, None if cfg is None else C.byref(cfg))
        if st != OK:
            raise RpfError(st, self._L.rpf_multi_last_error(self._h).decode())

    def set_membership(self, cfg):
        """rpf_multi_set_membership: the membership test of every slab (a function of the pixel alone: nothing moves per slab)"""
        st = self._L.rpf_multi_set_membership(self._h, None if cfg is None else C.byref(cfg))
        if st != OK:
            raise RpfError(st, self._L.rpf_multi_last_error(self._h).decode())

    def set_schedule(self, cfg):
        """rpf_multi_set_schedule: the same table on every slab (the passes of the call index it, and every slab runs them all)"""
        st = self._L.rpf_multi_set_schedule(self._h, None if cfg is None else C.byref(cfg))
        if st != OK:
            raise RpfError(st, self._L.rpf_multi_last_error(self._h).decode())

    def spike_stats(self):
        """rpf_multi_query_spike: SpikeStats of the most recent call, merged over the slabs"""
        s = SpikeStats()
        self._L.rpf_multi_query_spike(self._h, C.byref(s))
        return s

    def pass_report(self, pass_index):
        """rpf_multi_query_pass_report: the PassReport of that pass of the most recent call, merged over the slabs (the rows of
        every slab in image-row order, folded: the same numbers as one context; route and draws are the first slab's)"""
        r = PassReport()
        st = self._L.rpf_multi_query_pass_report(self._h, int(pass_index), C.byref(r))
        if st != OK:
            raise RpfError(st, self._L.rpf_multi_last_error(self._h).decode())
        return r

    def filter(self, planes, desc, ray_weight=None, allow_nonfinite=False):
        nd, _, _, pdt = dims(desc)
        planes = np.ascontiguousarray(planes, pdt)
        assert planes.shape == (nd, desc.H, desc.W, desc.S), planes.shape
        rw = None if ray_weight is None else np.ascontiguousarray(ray_weight, np.float32)
        srgb = np.empty((3, desc.H, desc.W, desc.S), np.float32)
        prgb = np.empty((desc.H, desc.W, 3), np.float32)
        st = self._L.rpf_multi_filter(self._h, C.byref(desc), _p(planes), _p(rw), _p(srgb), _p(prgb))
        if st != OK and not (allow_nonfinite and st == E_NONFINITE):
            raise RpfError(st, self._L.rpf_multi_last_error(self._h).decode())
        return srgb, prgb, st

    def filter_film(self, planes, desc, film, ray_weight=None, allow_nonfinite=False):
        """rpf_multi_filter_film: Context.filter_film for the whole image on every slab context; returns the same
        (sample_rgb, tile_rgb, tile_weight, image_rgb)"""
        nd, _, _, pdt = dims(desc)
        planes = np.ascontiguousarray(planes, pdt)
        assert planes.shape == (nd, desc.H, desc.W, desc.S), planes.shape
        rw = None if ray_weight is None else np.ascontiguousarray(ray_weight, np.float32)
        nx, ny = max(film.px1 - film.px0, 0), max(film.py1 - film.py0, 0)
        srgb = np.empty((3, desc.H, desc.W, desc.S), np.float32)
        tile, w, img = np.empty((ny, nx, 3), np.float32), np.empty((ny, nx), np.float32), np.empty((ny, nx, 3), np.float32)
        st = self._L.rpf_multi_filter_film(self._h, C.byref(desc), C.byref(film), _p(planes), _p(rw), _p(srgb), _p(tile),
                                           _p(w), _p(img))
        if st != OK and not (allow_nonfinite and st == E_NONFINITE):
            raise RpfError(st, self._L.rpf_multi_last_error(self._h).decode())
        return srgb, tile, w, img


def lds_bytes_required(S, box):
    return load().rpf_lds_bytes_required(S, box)
