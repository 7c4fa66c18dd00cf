#!/usr/bin/env python3
"""Scan gfx950 assembly of the kernel TUs for a miscompilation seen with hipcc 7.2: register-allocator spill code placed
at the top of a control-flow join block IN FRONT OF the instruction that re-enables the lanes masked off by the branch.
Those lanes never store their registers, and the reload after the join hands them whatever the scratch slot held (a
27-dim K = 25 kernel produced MI = +-inf that way, and one wild gather faulted).

Rule (round 3: any EXEC-restore form, any spill form): walking from a block label (.LBB*) to the first instruction that can
ENABLE lanes (s_or_b64 / s_mov_b64 / s_xor_b64 with exec as destination, s_or_saveexec / s_xor_saveexec), flag any scratch
store or reload (lines the compiler marks "Folded Spill" / "Folded Reload") and any v_accvgpr_write / v_accvgpr_read copy
met on the way, with nothing but waits, nops, scalar moves and SGPR spill traffic in between (round 2's scanner wanted the
spill code directly behind the label and directly in front of `s_or_b64 exec, exec`).  The walk stops without a verdict at
the first instruction doing real work (a value parked or fetched after that is the block's own business: e.g. an `if` body
that reads a parked operand and ends in its own s_or), at a branch, at the next label, or at an instruction that only
narrows EXEC (s_and / s_andn2 forms, or s_mov from a pair and-ed in the block: the head of an inner `if`).

Second rule: DPP read hazards.  The `row_newbcast` instructions of rpf_xlane.h sit in inline assembly, which neither the
compiler's hazard recogniser nor the assembler looks into; only the first read of a block carries its own `s_nop 1`.  The
hardware wants two wait states between a VALU write of a VGPR and a DPP read of it, and five between a VALU write of EXEC
and a DPP instruction.  For every `v_*_dpp ... row_newbcast` the scan walks back over the preceding instructions (one wait
state each, `s_nop N` counts N + 1; through labels and conditional branches along the fall-through path, up to an
unconditional branch or the head of the kernel) and flags a VALU instruction -- v_accvgpr_read included -- that writes a
register of the DPP source operand within two wait states, or EXEC within five.

Usage: check_spills.py [--report FILE] file.s [...]; exit status 1 if either is found.  --report writes, per
kernel, VGPR / AGPR / SGPR counts, LDS and scratch bytes, the compiler's spill counts (from the .amdgpu_metadata block of
the same assembly), the number of scratch spill instructions, and the static VALU / LDS / vector-memory / s_nop instruction
totals of the kernel's text: the resource usage of the build that ships."""
import re
import sys

# instructions that can ENABLE lanes (a join or an else flip): or / mov / xor into exec, s_or_saveexec.  Narrowing forms
# (s_and_b64 exec, s_andn2_b64 exec, s_and_saveexec_b64: the head of an inner `if`) end the walk without a verdict: code in
# front of them ran for exactly the lanes that go on to use it.
EXEC_WIDEN = re.compile(r"^(s_or_b64|s_mov_b64|s_xor_b64|s_xnor_b64|s_orn2_b64|s_cselect_b64|s_or_saveexec_b64|s_xor_saveexec_b64)\s+(exec|s\[\d+:\d+\], *exec|s\[\d+:\d+\],)")
EXEC_NARROW = re.compile(r"^(s_and_b64|s_andn2_b64)\s+exec\b|^s_(and|andn2)_saveexec_b64\b")
SPILL = re.compile(r"Folded Spill|Folded Reload")
ACC = re.compile(r"^v_accvgpr_(write|read)")
# instructions that may sit between the spill code and the EXEC restore without making the block "real work": waits, nops,
# scalar moves / address arithmetic that do not write EXEC, SGPR spill traffic (v_readlane / v_writelane ignore EXEC)
NEUTRAL = re.compile(r"^(s_waitcnt|s_nop|s_mov_b32|s_mov_b64\s+(?!exec)|s_add_|s_addc_|s_lshl|s_load|v_readlane_b32|v_writelane_b32|s_barrier)")
TERMINATOR = re.compile(r"^(s_cbranch|s_branch|s_endpgm|s_setpc)")


def scan(path):
    lines = open(path, errors="replace").read().split("\n")
    cur, bad, spills = None, {}, {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\S+):", l)
        if m:
            cur = m.group(1)
        if cur and "Folded Spill" in l:
            spills[cur] = spills.get(cur, 0) + 1
        if cur and l.startswith(".LBB"):
            j, n = i + 1, 0
            narrowed = set()  # SGPR pairs formed by s_and / s_andn2 inside this block: moving one into EXEC narrows it
            while j < len(lines):
                t = lines[j].strip()
                if not t or t.startswith(";"):
                    j += 1
                    continue
                if t.startswith(".LBB") or re.match(r"^_Z\S+:", t) or TERMINATOR.match(t):
                    break  # the block ends without touching EXEC: not a join with masked lanes
                m2 = re.match(r"^s_(and|andn2)_b64\s+(s\[\d+:\d+\]|vcc)\s*,", t)
                if m2:
                    narrowed.add(m2.group(2))
                m3 = re.match(r"^s_mov_b64\s+exec\s*,\s*(s\[\d+:\d+\]|vcc)", t)
                if EXEC_NARROW.match(t) or (m3 and m3.group(1) in narrowed):
                    break  # the head of an inner `if` (hipcc also writes it as s_mov s, exec; s_and t, s, cond; s_mov exec, t)
                if (EXEC_WIDEN.match(t) and re.match(r"^\S+\s+exec\b", t)) or re.match(r"^s_(or|xor)_saveexec_b64\b", t):
                    if n:
                        bad.setdefault(cur, []).append(i + 1)
                    break
                if SPILL.search(t) or ACC.match(t):
                    n += 1
                elif not NEUTRAL.match(t):
                    break  # real work starts before EXEC is touched: a value parked or fetched here is the block's own business
                j += 1
    return bad, spills


DPP_BCAST = re.compile(r"^v_\w+_dpp\s+(.*?)\s+row_newbcast")
VREG = re.compile(r"^v(\d+)$|^v\[(\d+):(\d+)\]$")
HARD_END = re.compile(r"^(s_branch|s_endpgm|s_setpc)")
TWO_DEST = re.compile(r"^(v_swap_b32|v_permlane\d+_swap)")  # both operands are written
DPP_VGPR_WAIT, DPP_EXEC_WAIT = 2, 5


def _vregs(op):
    m = VREG.match(op.strip())
    if not m:
        return set()
    if m.group(1) is not None:
        return {int(m.group(1))}
    return set(range(int(m.group(2)), int(m.group(3)) + 1))


def _instr(line):
    """the instruction of an assembly line ('' for labels, directives, comments and blank lines)"""
    t = line.split(";")[0].strip()
    if not t or t.startswith(".") or t.endswith(":"):
        return ""
    return t


def _operands(t):
    parts = t.split(None, 1)
    return [o.strip() for o in parts[1].split(",")] if len(parts) > 1 else []


def scan_dpp(path):
    """{kernel: [(line number, what)]}: VALU writes too close in front of a row_newbcast DPP read (see the module docstring)"""
    lines = open(path, errors="replace").read().split("\n")
    cur, bad = None, {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\S+):", l)
        if m:
            cur = m.group(1)
        t = _instr(l)
        d = DPP_BCAST.match(t) if t else None
        if not d:
            continue
        ops = _operands(t.split("row_newbcast")[0])
        src = _vregs(ops[1]) if len(ops) > 1 else set()
        ws, j = 0, i - 1
        while j >= 0 and ws < DPP_EXEC_WAIT:
            if re.match(r"^_Z\S+:", lines[j]):
                break  # the head of the kernel
            p = _instr(lines[j])
            j -= 1
            if not p:
                continue
            if HARD_END.match(p):
                break  # nothing falls through into the DPP from here
            n = re.match(r"^s_nop\s+(\d+)", p)
            if n:
                ws += int(n.group(1)) + 1
                continue
            if p.startswith("v_"):
                po = _operands(p)
                dst = _vregs(po[0]) if po else set()
                if TWO_DEST.match(p) and len(po) > 1:
                    dst |= _vregs(po[1])
                if ws < DPP_VGPR_WAIT and dst & src:
                    bad.setdefault(cur or "?", []).append((i + 1, "VALU write of the DPP source %d wait state(s) ahead (line %d)" % (ws, j + 2)))
                if p.startswith("v_cmpx") or (po and po[0] == "exec"):
                    bad.setdefault(cur or "?", []).append((i + 1, "VALU write of EXEC %d wait state(s) ahead (line %d)" % (ws, j + 2)))
            ws += 1
    return bad


def instruction_totals(path):
    """{kernel: (VALU, LDS, vector memory, s_nop)}: static instruction counts of each kernel's text"""
    out, cur = {}, None
    for l in open(path, errors="replace"):
        m = re.match(r"^(_Z\S+):", l)
        if m:
            cur = m.group(1)
            out[cur] = [0, 0, 0, 0]
            continue
        if cur is None:
            continue
        if l.startswith(".Lfunc_end"):
            cur = None
            continue
        t = _instr(l)
        if not t:
            continue
        if t.startswith("v_"):
            out[cur][0] += 1
        elif t.startswith("ds_"):
            out[cur][1] += 1
        elif t.startswith(("global_", "flat_", "buffer_", "scratch_")):
            out[cur][2] += 1
        elif t.startswith("s_nop"):
            out[cur][3] += 1
    return out


def metadata(path):
    """per-kernel resource figures from the .amdgpu_metadata block"""
    text = open(path, errors="replace").read()
    a, b = text.find(".amdgpu_metadata"), text.find(".end_amdgpu_metadata")
    out = {}
    if a < 0 or b < 0:
        return out
    for blk in re.split(r"\n  - \.agpr_count:", text[a:b])[1:]:
        blk = ".agpr_count:" + blk
        g = lambda k: (re.search(r"\." + k + r":\s*(\S+)", blk) or [None, "?"])[1]
        out[g("name")] = dict(vgpr=g("vgpr_count"), agpr=g("agpr_count"), sgpr=g("sgpr_count"), lds=g("group_segment_fixed_size"),
                              scratch=g("private_segment_fixed_size"), vspill=g("vgpr_spill_count"), sspill=g("sgpr_spill_count"),
                              wg=g("max_flat_workgroup_size"))
    return out


def demangle_short(name):
    m = re.search(r"(d19|d27)(\d+)(\w+?)(I.*)?E?v?NS_", name)
    # (d19::sched / d27::sched: the scheduled builds, RPF_IMPL_SCHED; ::listed and ::listed::sched: the listed ones, RPF_IMPL_LISTED)
    ns = re.search(r"3rpf\d+(d19|d27|generic)(6listed)?(5sched)?", name)
    k = re.search(r"kernelILi(\d+)ELb(\d)ELb(\d)ELi(\d)ELi(\d)E", name)
    base = re.search(r"\d+([a-z_]+kernel)", name)
    s = (ns.group(1) + "::" + ("listed::" if ns.group(2) else "") + ("sched::" if ns.group(3) else "") if ns else "") + (base.group(1) if base else name[:60])
    if k:
        s += "<K=%s,TL=%s,FAST=%s,NW=%s,PHASE=%s>" % k.groups()
    # the layout-generic kernels: the plane type, and FAST where a kernel has the fp32 stage-4 instantiation (RPF_FLAG_GENERIC_FAST)
    # ... and MEMBER where one has the membership test of RPF_FLAG_MEMBER_TEST in its stage 1b: the second flag of the wide kernel, the
    # only flag of the count kernels; LISTED where generic::filter_pixel_kernel reads listed members (its third parameter)
    t = re.search(r"3rpf7generic.*kernelI(f|6__half)(?:Lb([01])E)?(?:Lb([01])E)?E", name)
    if t:
        count = re.search(r"(wide|sampled)_count(_block|_mask|_list)?_kernel", name) is not None
        pixel = re.search(r"\d+filter_pixel_kernel", name) is not None
        fast = t.group(2) == "1" and not count
        member = (t.group(3) == "1" and not pixel) or (count and t.group(2) == "1")
        s += "<%s%s%s%s>" % ("float" if t.group(1) == "f" else "__half", ",FAST" if fast else "", ",MEMBER" if member else "",
                             ",LISTED" if pixel and t.group(3) == "1" else "")
    g = re.search(r"packed_kernelILi(\d+)E", name)
    if g:
        s += "<G=%s>" % g.group(1)
    t = re.search(r"3rpf7generic.*packed_kernelI(f|6__half)Li(\d+)E(?:Lb([01])E)?", name)  # ... and of their packed kernels the lanes per pixel
    if t:
        s += "<%s,G=%s%s>" % ("float" if t.group(1) == "f" else "__half", t.group(2), ",FAST" if t.group(3) == "1" else "")
    t = re.search(r"3rpf7generic.*filter_quad_kernelI(f|6__half)Li(\d+)E", name)  # ... of the four-wave kernels the own samples per sweep
    if t:
        s += "<%s,OWN=%s>" % ("float" if t.group(1) == "f" else "__half", t.group(2))
    return s


def main():
    args = sys.argv[1:]
    report = None
    if args and args[0] == "--report":
        report, args = args[1], args[2:]
    rc = 0
    rows = []
    for path in args:
        bad, spills = scan(path)
        meta = metadata(path)
        dpp = scan_dpp(path)
        tot = instruction_totals(path)
        for k, v in dpp.items():
            rc = 1
            for ln, what in v:
                print("%s: DPP READ HAZARD in %s at line %d: %s" % (path, k[:110], ln, what))
        for k, v in sorted(spills.items()):
            print("%s: %d scratch spill instructions in %s" % (path, v, k[:110]))
        for k, v in bad.items():
            rc = 1
            print("%s: SPILL CODE BEFORE EXEC RESTORE in %s at lines %s" % (path, k, v))
        for k, m in sorted(meta.items()):
            rows.append("%-58s VGPR %3s AGPR %3s SGPR %3s  LDS(static) %6s B  scratch %5s B/lane  spilled VGPR %3s SGPR %3s  spill-store instrs %3d  VALU %5d LDS %4d VMEM %4d s_nop %4d  %s"
                        % (demangle_short(k), m["vgpr"], m["agpr"], m["sgpr"], m["lds"], m["scratch"], m["vspill"], m["sspill"],
                           spills.get(k, 0), *tot.get(k, (0, 0, 0, 0)), "HAZARD" if (k in bad or k in dpp) else "ok"))
    if report:
        with open(report, "w") as f:
            f.write("# resource usage of the shipped build, per kernel (scripts/check_spills.py --report, written by build.py)\n"
                    "# LDS is dynamic for the fused kernels (see DESIGN.md section 4); 'HAZARD' = spill code in front of an EXEC restore, or a\n"
                    "# VALU write too close in front of a row_newbcast DPP read; VALU / LDS / VMEM / s_nop = static instruction totals\n")
            f.write("\n".join(rows) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
