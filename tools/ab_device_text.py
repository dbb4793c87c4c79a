#!/usr/bin/env python3
"""Is the device code of every .hip file the same as at another commit?  No GPU needed.

For every classpose_amd/csrc/*.hip the file is compiled twice with its own Makefile flags plus
`--offload-device-only --no-gpu-bundle-output -c`: once from `git archive REV` and once from the working tree.  Both
code objects are disassembled with llvm-objdump -d and compared as text without the two header lines (the raw bytes
differ by an embedded id).  One verdict line per file and flag set; exit status 1 when any text differs.

  tools/ab_device_text.py [--rev HEAD] [--debug cpx_net,cpx_net_f32,...] [--jobs 8] [cpx_net cpx_gemm ...]

--debug: the files compared under the -DCPX_DEBUG flags as well ("all" for every file).
"""
import argparse
import concurrent.futures as cf
import hashlib
import io
import os
import re
import shlex
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("classpose_amd", "csrc")


def objdump():
    for p in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump"), "llvm-objdump"):
        if os.path.sep not in p or os.path.exists(p):
            return p


def compile_lines():
    """{(name, debug): argv} from the Makefile's own rules"""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, CSRC), "-n", "-B", "all"], check=True, capture_output=True, text=True).stdout
    cmds = {}
    for line in out.splitlines():
        m = re.search(r"-c (\w+)\.hip -o (_build(?:_dbg)?)/", line)
        if m and line.startswith("hipcc"):
            cmds[(m.group(1), m.group(2) == "_build_dbg")] = shlex.split(line[:line.index(" -c ")])
    return cmds


def device_text(tree, name, argv, out_dir, tag):
    obj = os.path.join(out_dir, f"{name}.{tag}.co")
    subprocess.run(argv + ["--offload-device-only", "--no-gpu-bundle-output", "-c", name + ".hip", "-o", obj],
                   cwd=os.path.join(tree, CSRC), check=True, capture_output=True)
    text = subprocess.run([objdump(), "-d", obj], check=True, capture_output=True, text=True).stdout
    return "\n".join(text.splitlines()[2:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rev", default="HEAD")
    ap.add_argument("--debug", default="")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("names", nargs="*", help="only these files (default: every .hip file)")
    a = ap.parse_args()
    cmds = compile_lines()
    dbg = {n for n, _ in cmds} if a.debug == "all" else set(filter(None, a.debug.split(",")))
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "old")
        os.makedirs(old)
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.rev, CSRC, "include"], check=True, capture_output=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(old)
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", a.rev], check=True, capture_output=True, text=True).stdout.strip()
        jobs = sorted(k for k in cmds if not k[1] or k[0] in dbg)
        jobs = [k for k in jobs if os.path.exists(os.path.join(old, CSRC, k[0] + ".hip")) and (not a.names or k[0] in a.names)]
        with cf.ThreadPoolExecutor(a.jobs) as ex:
            fut = {(k, side): ex.submit(device_text, tree, k[0], cmds[k], tmp, f"{side}{int(k[1])}")
                   for k in jobs for side, tree in (("old", old), ("new", ROOT))}
            bad = 0
            for k in jobs:
                t0, t1 = fut[(k, "old")].result(), fut[(k, "new")].result()
                same = t0 == t1
                bad += not same
                print(f"device text vs {rev}  {k[0] + '.hip':24s} {'-DCPX_DEBUG' if k[1] else 'product    '}  "
                      f"{'identical' if same else 'DIFFERENT'}  {len(t1.splitlines())} lines  sha256 {hashlib.sha256(t1.encode()).hexdigest()[:16]}", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
