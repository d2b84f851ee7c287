#!/usr/bin/env python3
"""Instruction mix of the persistent sweep's batch loops (k_mf_resident, mfm_res.hpp), from the cross-compiled listing.

Compiles mfm_hip.hip device-only for gfx950 with _build.py's flags (-S), or reads a listing given with --asm, and prints for
every k_mf_resident instantiation: its VGPR count, scratch bytes and scratch instructions, and the instruction mix of the
code of sweeps A and B. The sweeps are found in one of two forms:
  - between the marker comments ";; res sweep A" / ";; res sweep B" / ";; res sweep end" that the kernel's empty
    asm statements leave in the listing (the on-chip groups of one sweep; a rolled batch loop in there is the code of 8
    slots that runs for 16);
  - failing those, as the innermost loops of at least 250 instructions (the rolled batch loops: two batches of 4 slots per
    iteration); a loop with ds_add_f64 is sweep A's, one without is sweep B's.
Usage: python scripts/res_isa.py [--asm FILE] [--keep FILE] [--all]

--same A.s B.s compares two listings of the same translation unit (say, before and after a change that claims to leave a
form's code alone): per k_mf_resident / k_res_score symbol whether the instruction streams and the .amdhsa_* resource lines are
equal; every other kernel must be in both, and a changed instruction count of one is reported. A plain comparison of the text
(comments, the __hip_cuid_* symbol and the function ordinal in local labels aside); exit status 1 on a difference or a missing
kernel, with the differing symbol and its first differing line. --full REGEX widens the symbols compared in full (default: the
sweep and the scorer; --full . compares every kernel of the translation unit, as a change that claims to touch no device code needs)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "myfm_amd", "csrc")

FP64 = re.compile(r"^v_(fma|add|mul)_f64")
CATS = ["total", "VALU", "v_cndmask", "fp64", "s_set_gpr_idx", "SALU other", "DS", "VMEM", "s_waitcnt", "scratch", "branch"]


def compile_listing(out):
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
             "-I" + CSRC]
    cmd = ["/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"] + flags + \
        ["--cuda-device-only", "-S", os.path.join(CSRC, "mfm_hip.hip"), "-o", out]
    subprocess.check_call(cmd)


def functions(lines):
    """name -> list of its lines (the instruction stream of every k_mf_resident)."""
    out, cur = {}, None
    for ln in lines:
        m = re.match(r"^(_Z\w*k_mf_resident\w*):", ln)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is not None:
            if ln.startswith(".Lfunc_end"):
                cur = None
                continue
            out[cur].append(ln)
    return out


def kernel_meta(lines):
    meta, cur = {}, None
    for ln in lines:
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            cur = m.group(1)
            meta[cur] = {}
            continue
        if cur is not None:
            m = re.match(r"^\s*\.amdhsa_(next_free_vgpr|private_segment_fixed_size|accum_offset)\s+(\d+)", ln)
            if m:
                meta[cur][m.group(1)] = int(m.group(2))
            if ".end_amdhsa_kernel" in ln:
                cur = None
    return meta


def kernels(path):
    """kernel symbol -> (its instructions and labels, comments stripped; its .amdhsa_* lines)"""
    text, meta, cur, cur_k = {}, {}, None, None
    with open(path) as f:
        for ln in f:
            m = re.match(r"^(\w+):", ln)
            if cur is None and m:  # (a function's label, or a data symbol's: those have no .amdhsa_kernel block and are dropped)
                cur = m.group(1)
                text[cur] = []
            elif ln.startswith(".Lfunc_end"):
                cur = None
            elif cur is not None:
                s = re.sub(r"\.L(BB|JTI)\d+_", r".L\1_", ln.split(";")[0].strip())  # (local labels carry the function's ordinal)
                if s and "__hip_cuid_" not in s:
                    text[cur].append(s)
            m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", ln)
            if m:
                cur_k = m.group(1)
                meta[cur_k] = []
            elif ".end_amdhsa_kernel" in ln:
                cur_k = None
            elif cur_k is not None:
                meta[cur_k].append(ln.strip())
    return {k: (text[k], meta[k]) for k in meta if k in text}


def same(path_a, path_b, full="k_mf_resident|k_res_score"):
    a, b = kernels(path_a), kernels(path_b)
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("MISSING in %s: %s" % (path_a if name not in a else path_b, name))
            bad += 1
            continue
        n_a, n_b = (sum(1 for x in k[name][0] if not x.endswith(":") and not x.startswith(".")) for k in (a, b))
        if not re.search(full, name):
            if n_a != n_b:  # (reported, not counted: the exit status speaks of the kernels that --full names)
                print("other kernel, %d -> %d instructions: %s" % (n_a, n_b, name))
            continue
        for what, x, y in (("instruction stream", a[name][0], b[name][0]), ("resources", a[name][1], b[name][1])):
            if x != y:
                i = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
                print("DIFFERENT %s: %s\n  line %d: %r\n      vs: %r" % (what, name, i, x[i] if i < len(x) else None, y[i] if i < len(y) else None))
                bad += 1
                break
        else:
            print("equal (%d instructions, %d resource lines): %s" % (n_a, len(a[name][1]), name))
    print("%d kernels compared, %d differ" % (len(set(a) | set(b)), bad))
    return 1 if bad else 0


def is_insn(ln):
    s = ln.strip()
    return bool(s) and not s.startswith((";", ".", "//")) and not s.endswith(":")


def mnemonic(ln):
    return ln.strip().split()[0]


def mix(insns):
    c = dict.fromkeys(CATS, 0)
    for ln in insns:
        op = mnemonic(ln)
        c["total"] += 1
        if op.startswith("v_"):
            c["VALU"] += 1
            if op.startswith("v_cndmask"):
                c["v_cndmask"] += 1
            if FP64.match(op):
                c["fp64"] += 1
        elif op.startswith("s_set_gpr_idx"):
            c["s_set_gpr_idx"] += 1
        elif op.startswith("s_waitcnt"):
            c["s_waitcnt"] += 1
        elif op.startswith(("s_branch", "s_cbranch")):
            c["branch"] += 1
        elif op.startswith("s_"):
            c["SALU other"] += 1
        elif op.startswith("ds_"):
            c["DS"] += 1
        elif op.startswith("scratch_"):
            c["scratch"] += 1
        elif op.startswith(("global_", "buffer_", "flat_")):
            c["VMEM"] += 1
    return c


def marked_regions(body):
    """{'A': [...], 'B': [...]} between the sweep markers (first occurrence of each), or None."""
    regs, cur = {}, None
    for ln in body:
        m = re.search(r";; res sweep (A|B|end)\b", ln)
        if m:
            cur = None if m.group(1) == "end" or m.group(1) in regs else m.group(1)
            if cur:
                regs[cur] = []
            continue
        if cur and (is_insn(ln) or "This Inner Loop Header" in ln):
            regs[cur].append(ln)
    return regs or None


def inner_loops(body):
    """innermost loops: header label -> instructions of all blocks of the loop."""
    loops, cur = {}, None
    for i, ln in enumerate(body):
        if not (re.match(r"^\.LBB\w+:", ln) or ln.startswith("; %bb")):
            if cur and is_insn(ln):
                loops[cur].append(ln)
            continue
        note, j = ln, i + 1  # (a block's loop notes may go on over comment-only lines)
        while j < len(body) and re.match(r"^\s+;", body[j]):
            note += body[j]
            j += 1
        if "This Inner Loop Header" in note:
            cur = re.match(r"^\.(LBB\w+):", ln).group(1)
            loops.setdefault(cur, [])
            continue
        m = re.findall(r"in Loop: Header=(BB\w+)", note)
        cur = "L" + m[-1] if m and ("L" + m[-1]) in loops else None
    return loops


def row(label, c, per):
    return "  %-26s" % label + "".join("%9.1f" % (c[k] / per) if per != 1 else "%9d" % c[k] for k in CATS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", help="read this listing instead of compiling")
    ap.add_argument("--keep", help="write the compiled listing here")
    ap.add_argument("--all", action="store_true", help="every instantiation (default: <512,4,1,...> in all its forms: OVF, XCH, S2B)")
    ap.add_argument("--same", nargs=2, metavar=("A.s", "B.s"), help="compare two listings kernel by kernel")
    ap.add_argument("--full", default="k_mf_resident|k_res_score", metavar="REGEX",
                    help="with --same: the kernels whose streams and resources are compared in full ('.': all)")
    args = ap.parse_args()
    if args.same:
        return same(*args.same, full=args.full)
    path = args.asm
    if not path:
        path = args.keep or os.path.join(tempfile.mkdtemp(prefix="res_isa_"), "mfm_hip.s")
        compile_listing(path)
    with open(path) as f:
        lines = f.read().splitlines()
    funcs, meta = functions(lines), kernel_meta(lines)
    print("%-28s" % "" + "".join("%9s" % k[:9] for k in CATS))
    for name in sorted(funcs):
        m = re.search(r"ILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELb(\d)E(?:Lb(\d)E)?", name)  # (the sixth flag, S2B: from its introduction on)
        tag = "<%s>" % ",".join([m.group(1), m.group(2), m.group(3)] +
                                ["true" if b == "1" else "false" for b in m.groups()[3:] if b is not None]) if m else name
        if not args.all and not (m and m.group(2) == "4" and m.group(3) == "1"):
            continue
        body = funcs[name]
        km = meta.get(name, {})
        nscr = sum(1 for ln in body if is_insn(ln) and mnemonic(ln).startswith("scratch_"))
        print("k_mf_resident%s: VGPRs %s (arch %s), scratch %s B, scratch instructions %d, %d instructions in all" % (
            tag, km.get("next_free_vgpr", "?"), km.get("accum_offset", "?"), km.get("private_segment_fixed_size", "?"), nscr,
            sum(1 for ln in body if is_insn(ln))))
        regs = marked_regions(body)
        if regs:
            slots = 16 * (int(m.group(2)) + int(m.group(3))) if m else 1
            for k in sorted(regs):
                c = mix(regs[k])
                # a rolled batch loop inside the region: its body is the code of 8 slots, and stands for 16
                nloop = sum(1 for ln in regs[k] if "This Inner Loop Header" in ln)
                code_slots = slots - 8 * nloop
                print(row("sweep %s (code of %d slots)" % (k, code_slots), c, 1))
                print(row("sweep %s per slot" % k, c, code_slots))
        else:
            for hdr, ins in inner_loops(body).items():
                if len(ins) < 250:
                    continue
                c = mix(ins)
                kind = "A" if any(mnemonic(x).startswith("ds_add") for x in ins) else "B"
                print(row("loop %s %s / 8 slots" % (hdr, kind), c, 1))
                print(row("loop %s %s per slot" % (hdr, kind), c, 8))


if __name__ == "__main__":
    sys.exit(main())
