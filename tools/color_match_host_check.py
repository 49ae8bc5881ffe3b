"""Build tools/color_match_host.cpp with the host sanitizers and run it over the colour-matching case list.

    python tools/color_match_host_check.py [--cxx c++] [--keep DIR]

Writes every case of tests/_color_cases.case_groups(), in both modes, with the numpy model's output and gains as its expectation
into one file, compiles the program with -fsanitize=address,undefined (host code only, a program of its own: nothing is loaded
into Python, nothing touches a GPU) and runs it.  Exit status 0: every case equals the model, out of place and in place, and the
sanitizers reported nothing (-fno-sanitize-recover: a report ends the program with a failure)."""
import argparse
import os
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _color_cases as CC  # noqa: E402


def write_cases(path):
    """the case file of tools/color_match_host.cpp; returns the number of cases"""
    blocks = []
    for S, group in CC.case_groups():
        for name, (pred, ref) in group.items():
            for mode, code in CC.MODES.items():
                want, info = CC.model(pred, ref, mode)
                blocks.append(struct.pack("<5i", S, code, *[ch["g"] for ch in info]) + pred.tobytes() + ref.tobytes() + want.tobytes())
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(blocks)))
        for b in blocks:
            f.write(b)
    return len(blocks)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cxx", default=os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++"))
    ap.add_argument("--keep", default=None, help="write the files here and keep them")
    a = ap.parse_args()
    if not a.cxx:
        print("no host C++ compiler")
        return 2
    with tempfile.TemporaryDirectory() as tmp:
        d = a.keep or tmp
        os.makedirs(d, exist_ok=True)
        cases = os.path.join(d, "cases.bin")
        n = write_cases(cases)
        exe = os.path.join(d, "color_match_host")
        # the sanitizer runtimes linked INTO the program (clang's default, gcc's by flag): it runs as it is, whatever else is loaded
        static = [] if "clang" in os.path.basename(a.cxx) else ["-static-libasan", "-static-libubsan"]
        cmd = [a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + [
            os.path.join(ROOT, "tools", "color_match_host.cpp"), "-o", exe]
        print(" ".join(cmd))
        subprocess.run(cmd, check=True)
        print("%d cases" % n)
        sys.stdout.flush()
        rc = subprocess.run([exe, cases]).returncode
        print("exit status %d" % rc)
        return rc


if __name__ == "__main__":
    sys.exit(main())
