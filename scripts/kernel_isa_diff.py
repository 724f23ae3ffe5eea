#!/usr/bin/env python3
"""Compare two device assembly listings kernel by kernel.

    hipcc --offload-arch=gfx950 <the library's flags> --cuda-device-only -S -o X.s ba_solver.hip
    kernel_isa_diff.py OLD.s NEW.s [--touched k_pcg_cam,k_mc_cam,...]

A kernel runs from its `_Z...:` label to the next `.Lfunc_end`; comments and blank lines are dropped and the function's number is taken
out of its local labels (.LBB12_3 -> .LBB_3), so a body is "identical" when every instruction, label and descriptor line is.  For a body
that differs the script prints the histogram of floating-point arithmetic opcodes of both versions -- v_ fma / mul / add / sub / div* /
rcp / rsq / sqrt / pk_* on f32 / f64, the encoding suffix (_e32, _e64, _dpp, _sdwa) dropped and fmac counted as fma, subrev as sub,
since those are the register allocator's choice, not the arithmetic's -- and both versions' .amdhsa_next_free_vgpr, .amdhsa_accum_offset
and private-segment size.  Equal histograms mean that no contraction or reassociation changed.

With --touched (kernel names as in the source, any instantiation) the exit status is 1 when the symbol sets differ, when a kernel that
is not listed differs, or when a listed one changes its histogram or gains a private segment; without it the script only reports.
"""
import argparse
import collections
import re
import sys

LABEL = re.compile(r"^(_Z\w+):")
LOCAL = re.compile(r"\.L(BB|func_end|func_begin|tmp)\d+")
ENCODING = re.compile(r"(_e32|_e64|_dpp|_sdwa)+$")
FP_OP = re.compile(r"^v_(pk_[a-z]+|fma|mul|mul_legacy|add|sub|div_[a-z]+|rcp|rcp_iflag|rsq|sqrt)_(f32|f64)$")
RESOURCES = (".amdhsa_next_free_vgpr", ".amdhsa_accum_offset", ".amdhsa_private_segment_fixed_size")


def kernels(path):
    """{symbol: [body lines]} of a listing"""
    out, name, body = {}, None, None
    with open(path) as f:
        for raw in f:
            line = raw.split(";", 1)[0].strip()
            if name is None:
                m = LABEL.match(line)
                if m:
                    name, body = m.group(1), []
                continue
            if line.startswith(".Lfunc_end"):
                out[name], name = body, None
            elif line:
                body.append(LOCAL.sub(lambda m: ".L" + m.group(1), line))
    return out


def fp_histogram(body):
    h = collections.Counter()
    for line in body:
        op = ENCODING.sub("", line.split(None, 1)[0]).replace("v_fmac_", "v_fma_").replace("v_subrev_", "v_sub_")
        if FP_OP.match(op):
            h[op] += 1
    return h


def resources(body):
    r = dict.fromkeys(RESOURCES, None)
    for line in body:
        w = line.split()
        if len(w) == 2 and w[0] in r:
            r[w[0]] = int(w[1])
    return r


def source_name(symbol):
    """k_name of a mangled kernel symbol: _Z<len><name>..."""
    m = re.match(r"_Z(\d+)", symbol)
    return symbol[m.end():m.end() + int(m.group(1))] if m else symbol


def compare(old, new, touched=None, out=sys.stdout):
    """prints the report; the number of findings against `touched` (0 when it is None)"""
    bad = 0
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    print("kernels: %d old, %d new; symbol sets %s" % (len(old), len(new), "equal" if not (only_old or only_new) else "DIFFER"), file=out)
    for s in only_old:
        print("  only in old: %s" % s, file=out)
    for s in only_new:
        print("  only in new: %s" % s, file=out)
    bad += len(only_old) + len(only_new)
    same = differ = 0
    for s in sorted(set(old) & set(new)):
        if old[s] == new[s]:
            same += 1
            print("identical  %s" % s, file=out)
            continue
        differ += 1
        ho, hn = fp_histogram(old[s]), fp_histogram(new[s])
        ro, rn = resources(old[s]), resources(new[s])
        listed = touched is not None and source_name(s) in touched
        print("DIFFERS    %s  (%d -> %d lines)%s" % (s, len(old[s]), len(new[s]), "" if touched is None or listed else "  NOT LISTED"), file=out)
        print("  fp opcodes %s" % ("equal" if ho == hn else "DIFFER"), file=out)
        for op in sorted(set(ho) | set(hn)):
            print("    %-24s %5d %5d%s" % (op, ho[op], hn[op], "" if ho[op] == hn[op] else "  <--"), file=out)
        for k in RESOURCES:
            print("  %-36s %5s %5s" % (k, ro[k], rn[k]), file=out)
        if touched is not None and (not listed or ho != hn or (rn[RESOURCES[2]] or 0) > (ro[RESOURCES[2]] or 0)):
            bad += 1
    print("bodies: %d identical, %d differ" % (same, differ), file=out)
    return bad if touched is not None else 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--touched", help="comma-separated kernel names that may differ (with equal fp opcode histograms)")
    a = ap.parse_args(argv)
    touched = set(a.touched.split(",")) if a.touched is not None else None
    return 1 if compare(kernels(a.old), kernels(a.new), touched) else 0


if __name__ == "__main__":
    sys.exit(main())
