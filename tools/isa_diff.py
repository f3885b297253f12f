#!/usr/bin/env python3
"""Per-kernel comparison of two trees' gfx950 device assembly (a refactor's check that no kernel changed).

Compile every translation unit of both trees with the Makefile's flags plus
    -fuse-cuid=none --cuda-device-only -S <unit>.hip -o <dir>/<unit>.s
(-fuse-cuid=none: the __hip_cuid_* symbol is otherwise random per compile), then
    python3 tools/isa_diff.py <parent-dir> <new-dir> [--show N]
prints one line per translation unit (kernel count, identical or not) and, for each kernel whose code differs, its
VGPR / AGPR / SGPR counts, private segment, LDS and code size in both trees and whether the sequence of MFMA and
s_barrier instructions is the same. --show N prints the first N differing lines of each such kernel."""
import difflib
import os
import re
import sys

RES = [("vgpr", r"\.amdhsa_next_free_vgpr\s+(\d+)"), ("accum_offset", r"\.amdhsa_accum_offset\s+(\d+)"),
       ("agpr", r"; NumAgprs:\s+(\d+)"), ("sgpr", r"\.amdhsa_next_free_sgpr\s+(\d+)"),
       ("private", r"\.amdhsa_private_segment_fixed_size\s+(\d+)"), ("lds", r"\.amdhsa_group_segment_fixed_size\s+(\d+)"),
       ("code_bytes", r"; codeLenInByte = (\d+)")]


def kernels(path):
    """{symbol: text from the kernel's label to its .end_amdhsa_kernel}"""
    s = "".join(l for l in open(path) if "__hip_cuid" not in l)
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)$", s, re.M):
        name = m.group(1)
        st = s.find("\n" + name + ":")
        en = s.find(".end_amdhsa_kernel", m.end())
        info = s.find("; Occupancy:", en)  # the "; Kernel info:" comments (code size, AGPRs) follow the descriptor
        out[name] = s[st + 1:info if 0 <= info < en + 4000 else en]
    return out


def code_of(text):
    # the whole function (a kernel with early exits has several s_endpgm), without the labels' function numbering
    # (.LBB12_3 -> .LBB_3) and the comments
    end = text.find(".Lfunc_end")
    body = text[:end] if end >= 0 else text
    return [re.sub(r"\.L(BB|func_end|tmp)\d+", r".L\1", l.split(";")[0].rstrip()) for l in body.splitlines()]


def resources(text):
    return {k: (int(m.group(1)) if (m := re.search(p, text)) else None) for k, p in RES}


def pipeline(code):
    return [l.split()[0] for l in code if re.match(r"\s*(v_mfma|s_barrier)", l)]


def main():
    pa, pb = sys.argv[1], sys.argv[2]
    show = int(sys.argv[sys.argv.index("--show") + 1]) if "--show" in sys.argv else 0
    bad = 0
    fa, fb = ({x for x in os.listdir(d) if x.endswith(".s")} for d in (pa, pb))
    for f in sorted(fa ^ fb):
        bad += 1
        print(f"{f[:-2]}: only in {pa if f in fa else pb}")
    for f in sorted(fa & fb):
        ka, kb = kernels(os.path.join(pa, f)), kernels(os.path.join(pb, f))
        diff = [k for k in ka if k in kb and code_of(ka[k]) != code_of(kb[k])]
        res_only = [k for k in ka if k in kb and k not in diff and resources(ka[k]) != resources(kb[k])]
        gone, new = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
        same = not (diff or res_only or gone or new)
        bad += not same
        print(f"{f[:-2]}: {len(ka)} kernels, " + ("identical" if same else
              f"{len(diff)} differ, {len(res_only)} differ in resources only, {len(gone)} removed, {len(new)} added"))
        for k in gone:
            print(f"  removed {k}")
        for k in new:
            print(f"  added {k}")
        for k in diff + res_only:
            ca, cb = code_of(ka[k]), code_of(kb[k])
            print(f"  {k}\n    parent {resources(ka[k])}\n    new    {resources(kb[k])}\n"
                  f"    MFMA / s_barrier sequence {'same' if pipeline(ca) == pipeline(cb) else 'DIFFERENT'}")
            if show:
                print("\n".join(list(difflib.unified_diff(ca, cb, "parent", "new", lineterm="", n=1))[:show]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
