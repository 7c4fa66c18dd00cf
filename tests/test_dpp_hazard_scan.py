"""scripts/check_spills.py, second rule: a VALU write of a row_newbcast DPP read's source register needs two wait states in
front of the read, a VALU write of EXEC five (the reads sit in inline assembly, where no tool inserts them)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN = os.path.join(ROOT, "scripts", "check_spills.py")

DPP = "\tv_fmac_f64_dpp v[10:11], v[4:5], v[20:21] row_newbcast:3 row_mask:0xf bank_mask:0xf\n"
MOV = "\tv_mov_b64_dpp v[10:11], v[4:5] row_newbcast:15 row_mask:0xf bank_mask:0xf\n"
HEAD, TAIL = "_Zk:\n.LBB0_1:\n", "\ts_endpgm\n.Lfunc_end0:\n"

CASES = {
    # planted hazards
    "hazard_copy": (HEAD + "\tv_mov_b32_e32 v5, v9\n" + DPP + TAIL, 1),
    "hazard_acc_reload": (HEAD + "\tv_accvgpr_read_b32 v4, a7\n\ts_waitcnt lgkmcnt(0)\n" + DPP + TAIL, 1),
    "hazard_pair_write": (HEAD + "\tv_add_f64 v[4:5], v[6:7], v[8:9]\n\ts_nop 0\n" + MOV + TAIL, 1),
    "hazard_across_label": ("_Zk:\n\tv_mov_b32_e32 v4, v9\n.LBB0_1:\n" + DPP + TAIL, 1),
    "hazard_exec": (HEAD + "\tv_cmpx_lt_f64_e32 v[6:7], v[8:9]\n\ts_nop 1\n\ts_mov_b32 s5, 0\n" + DPP + TAIL, 1),
    # the same texts with the wait states in between
    "ok_copy_nop": (HEAD + "\tv_mov_b32_e32 v5, v9\n\ts_nop 1\n" + DPP + TAIL, 0),
    "ok_acc_reload_nop": (HEAD + "\tv_accvgpr_read_b32 v4, a7\n\ts_waitcnt lgkmcnt(0)\n\ts_nop 0\n" + DPP + TAIL, 0),
    "ok_two_instructions": (HEAD + "\tv_add_f64 v[4:5], v[6:7], v[8:9]\n\ts_mov_b32 s5, 0\n\tv_mov_b32_e32 v30, v31\n" + MOV + TAIL, 0),
    "ok_exec_nop": (HEAD + "\tv_cmpx_lt_f64_e32 v[6:7], v[8:9]\n\ts_nop 4\n" + DPP + TAIL, 0),
    # clean blocks: writes of other registers, the accumulator of the previous DPP, a load (waited for, not a VALU write)
    "ok_clean": (HEAD + "\tv_mov_b32_e32 v6, v9\n\tv_add_f64 v[20:21], v[6:7], v[8:9]\n" + DPP +
                 "\tv_fmac_f64_dpp v[12:13], v[4:5], v[22:23] row_newbcast:4 row_mask:0xf bank_mask:0xf\n" + TAIL, 0),
    "ok_lds_read": (HEAD + "\tds_read_b64 v[4:5], v40\n\ts_waitcnt lgkmcnt(0)\n" + DPP + TAIL, 0),
    "ok_behind_branch": ("_Zk:\n\tv_mov_b32_e32 v4, v9\n\ts_branch .LBB0_2\n.LBB0_1:\n" + DPP + TAIL, 0),
}


def test_dpp_hazard_scanner_rules(tmp_path):
    for name, (txt, want) in CASES.items():
        f = tmp_path / (name + ".s")
        f.write_text(txt)
        r = subprocess.run([sys.executable, SCAN, str(f)], stdout=subprocess.PIPE, text=True)
        assert r.returncode == want, (name, r.stdout)
        assert ("DPP READ HAZARD" in r.stdout) == bool(want), (name, r.stdout)


def test_report_carries_instruction_totals(tmp_path):
    """--report: the static VALU / LDS / vector-memory / s_nop totals of each kernel's text stand in its row"""
    meta = ("\t.amdgpu_metadata\n---\namdhsa.kernels:\n  - .agpr_count:     0\n    .group_segment_fixed_size: 0\n"
            "    .max_flat_workgroup_size: 64\n    .name:           _Zk\n    .private_segment_fixed_size: 0\n    .sgpr_count:     10\n"
            "    .sgpr_spill_count: 0\n    .vgpr_count:     24\n    .vgpr_spill_count: 0\n...\n\t.end_amdgpu_metadata\n")
    body = (HEAD + "\tglobal_load_dword v1, v2, s[0:1]\n\tds_read_b64 v[4:5], v40\n\ts_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_nop 1\n" + DPP +
            "\tv_add_f64 v[20:21], v[6:7], v[8:9]\n\tds_write_b64 v40, v[20:21]\n" + TAIL)
    f, rep = tmp_path / "k.s", tmp_path / "report.txt"
    f.write_text(body + meta)
    assert subprocess.run([sys.executable, SCAN, "--report", str(rep), str(f)], stdout=subprocess.PIPE).returncode == 0
    row = [l for l in rep.read_text().split("\n") if l and not l.startswith("#")]
    assert len(row) == 1 and "VALU     2 LDS    2 VMEM    1 s_nop    1" in row[0] and row[0].endswith("ok"), row
