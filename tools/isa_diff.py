#!/usr/bin/env python3
"""Which device kernels changed between a git revision and the working tree?

    python tools/isa_diff.py <rev> [file.hip ...]

Compiles csrc/<file> of <rev> and of the working tree for gfx950 with the flags of q-diffusion_amd/build.py
(`--save-temps`-free: `-S --cuda-device-only`), splits the device assembly into functions and compares the instruction
streams symbol by symbol (labels renumbered, comments and debug directives dropped).  The symbols of all files given are
pooled on each side, so a kernel that moved from one file to another is compared (name both files); a file absent from <rev>
contributes nothing to the old side.  Used at the end of a round whose
last commits could not be run on a GPU: a default-path kernel whose instruction stream is IDENTICAL to the last
GPU-verified revision needs no new verification; only the listed ones do.
Objects go to q-diffusion_amd/build/isa_diff/ (git-ignored)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "q-diffusion_amd"))
import build as B  # noqa: E402

OUT = os.path.join(ROOT, "q-diffusion_amd", "build", "isa_diff")


def device_asm(src_path, inc_dirs, out_path):
    cmd = [B._hipcc()] + B.CFLAGS + [f"-I{d}" for d in inc_dirs] + ["-x", "hip", "--cuda-device-only", "-S", src_path, "-o", out_path]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    return open(out_path).read()


def functions(asm):
    """{symbol: [normalised instruction lines]} of every function in a device .s file."""
    fns, cur, name = {}, None, None
    for line in asm.splitlines():
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", line)
        if m and not m.group(1).startswith((".L", "BB", "Lfunc")):
            name, cur = m.group(1), []
            fns[name] = cur
            continue
        if cur is None:
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith((".loc", ".file", ".cfi", ".p2align", ".Ltmp", ".Lfunc", ".size", ".type", ".section", ".text")):
            if s.startswith(".size"):
                cur = None
            continue
        cur.append(s)
    # local labels are numbered per function: basic blocks, and the anchors of relaxed long branches (.Lpost_getpcN, a counter
    # that runs over the whole file and so follows the order in which the kernels were instantiated)
    local = r"\.LBB\w+|\.Lpost_getpc\d+"
    norm = {}
    for k, lines in fns.items():
        labels, out = {}, []
        for s in lines:
            m = re.match(rf"^({local}):$", s)
            if m:
                labels.setdefault(m.group(1), f"L{len(labels)}")
        for s in lines:
            out.append(re.sub(local, lambda mm: labels.get(mm.group(0), mm.group(0)), s))
        norm[k] = out
    return norm


def main():
    rev = sys.argv[1]
    files = sys.argv[2:] or [s for s in B.SOURCES if s.endswith(".hip")]
    os.makedirs(OUT, exist_ok=True)
    old_root = os.path.join(OUT, "old")
    os.makedirs(os.path.join(old_root, "csrc"), exist_ok=True)
    os.makedirs(os.path.join(OUT, "include"), exist_ok=True)
    # common.h includes "../../include/qdiff_hip.h": two levels above old/csrc/ is OUT
    for rel, dst in (("q-diffusion_amd/csrc/common.h", os.path.join(old_root, "csrc", "common.h")),
                     ("include/qdiff_hip.h", os.path.join(OUT, "include", "qdiff_hip.h"))):
        open(dst, "w").write(subprocess.run(["git", "show", f"{rev}:{rel}"], cwd=ROOT, capture_output=True, text=True, check=True).stdout)
    # every header of the old csrc/ beside common.h (a header absent from <rev> is simply not there for the old sources)
    for h in os.listdir(B.CSRC):
        if h.endswith(".h") and h != "common.h":
            r = subprocess.run(["git", "show", f"{rev}:q-diffusion_amd/csrc/{h}"], cwd=ROOT, capture_output=True, text=True)
            dst = os.path.join(old_root, "csrc", h)
            if r.returncode == 0:
                open(dst, "w").write(r.stdout)
            elif os.path.exists(dst):                    # (left by a run against another revision)
                os.remove(dst)
    # symbols are pooled over all files, on each side: a kernel that moved between files is compared, not "removed" and "new"
    a, b, home, old_home = {}, {}, {}, {}
    for f in files:
        new_src = os.path.join(B.CSRC, f)
        if os.path.exists(new_src):
            fb = functions(device_asm(new_src, [B.CSRC], os.path.join(OUT, f + ".new.s")))
            b.update(fb)
            for k in fb:
                home.setdefault(k, f)
        else:
            print(f"{f}: not in the working tree (removed file)")
        r = subprocess.run(["git", "show", f"{rev}:q-diffusion_amd/csrc/{f}"], cwd=ROOT, capture_output=True, text=True)
        if r.returncode != 0:
            print(f"{f}: not in {rev} (new file)")
            continue
        old_src = os.path.join(old_root, "csrc", f)
        open(old_src, "w").write(r.stdout)
        fa = functions(device_asm(old_src, [os.path.join(old_root, "csrc")], os.path.join(OUT, f + ".old.s")))
        a.update(fa)
        old_home.update({k: f for k in fa if k not in old_home})
    home.update({k: f for k, f in old_home.items() if k not in home})
    # (__hip_cuid_<hash>: the per-compilation-unit id symbol, another name for every source text)
    a, b = ({k: v for k, v in side.items() if not k.startswith("__hip_cuid_")} for side in (a, b))
    diff = [k for k in a if k in b and a[k] != b[k]]
    gone, new = [k for k in a if k not in b], [k for k in b if k not in a]
    # a symbol counts under the first file given that holds it now (a removed one: that held it); the metadata headers every
    # file has (amdhsa.kernels, amdhsa.version) are pooled like any symbol, so they count once
    for f in files:
        def here(ks):
            return [k for k in ks if home[k] == f]
        same = here(k for k in a if k in b and a[k] == b[k])
        print(f"{f}: {len(same)} kernels identical, {len(here(diff))} changed, {len(here(new))} new, {len(here(gone))} removed")
        for k in here(diff):
            n = sum(1 for x, y in zip(a[k], b[k]) if x != y) + abs(len(a[k]) - len(b[k]))
            print(f"   CHANGED {k}  ({len(a[k])} -> {len(b[k])} lines, ~{n} differ)")
        for k in here(new):
            print(f"   new     {k}")
        for k in here(gone):
            print(f"   removed {k}")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
