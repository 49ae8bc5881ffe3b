"""Build tools/jpeg_decode_host.cpp with the host sanitizers and run it over the decoder's valid files and its corrupt corpus.

    python tools/jpeg_decode_host_check.py [--cxx c++] [--keep DIR]

Writes every file of tests/_jpeg_decode_cases.files() with PIL's decoded pixels as its expectation (.npy), every file of
altered_files() with the reference's pixels, and every file of corrupt_corpus(), compiles the program with
-fsanitize=address,undefined (host code only, a program of its own: nothing is loaded into Python, nothing touches a GPU) and runs it.  Exit status 0: every valid file decoded to PIL's pixels, every corrupt
file was refused, and the sanitizers reported nothing (-fno-sanitize-recover: a report ends the program with a failure)."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _jpeg_decode_cases as dc  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cxx", default=os.environ.get("CXX", "c++"))
    ap.add_argument("--keep", default=None, help="write the files here and keep them")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        d = a.keep or tmp
        os.makedirs(d, exist_ok=True)
        lines = []
        for name, data in dc.files():
            jpg, npy = os.path.join(d, name + ".jpg"), os.path.join(d, name + ".npy")
            open(jpg, "wb").write(data)
            np.save(npy, dc.expected(name, data))
            lines.append("valid %s %s" % (jpg, npy))
        for name, data, img in dc.altered_files():      # overwrites that stay decodable: the strict reference's own pixels
            jpg, npy = os.path.join(d, name + ".jpg"), os.path.join(d, name + ".npy")
            open(jpg, "wb").write(data)
            np.save(npy, img)
            lines.append("valid %s %s" % (jpg, npy))
        for name, data, _ in dc.corrupt_corpus():
            jpg = os.path.join(d, "corrupt_" + name + ".jpg")
            open(jpg, "wb").write(data)
            lines.append("corrupt %s -" % jpg)
        manifest = os.path.join(d, "manifest.txt")
        open(manifest, "w").write("\n".join(lines) + "\n")
        exe = os.path.join(d, "jpeg_decode_host")
        cmd = [a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
               os.path.join(ROOT, "tools", "jpeg_decode_host.cpp"), "-o", exe]
        print(" ".join(cmd))
        subprocess.run(cmd, check=True)
        rc = subprocess.run([exe, manifest]).returncode
        print("exit status %d" % rc)
        return rc


if __name__ == "__main__":
    sys.exit(main())
