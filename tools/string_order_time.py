#!/usr/bin/env python3
"""Times the device ranking of a string sort key against the host ranking (tools/string_order_time.cpp, through the C++ mirror) and writes
profiles/string_order.txt.  Needs the library built (__graft_entry__.build()) and an MI355X.  Usage: tools/string_order_time.py [output file]"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    source = os.path.join(ROOT, "tools", "string_order_time.cpp")
    binary = os.path.join(ROOT, "tools", "string_order_time_bin")
    deps = [source, os.path.join(ROOT, "hyrise_amd", "host", "hyrise_host.hpp"), os.path.join(ROOT, "hyrise_amd", "libhyrise_amd.so")]
    if not os.path.exists(binary) or any(os.path.getmtime(d) > os.path.getmtime(binary) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unused-function", "-o", binary, source, "-L" + os.path.join(ROOT, "hyrise_amd"), "-lhyrise_amd",
                               "-Wl,-rpath,$ORIGIN/../hyrise_amd"], cwd=ROOT)
    if "--build-only" in sys.argv:
        return
    arguments = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = arguments[0] if arguments else os.path.join(ROOT, "profiles", "string_order.txt")
    text = subprocess.run([binary], stdout=subprocess.PIPE, text=True, check=True).stdout
    print(text)
    with open(out, "w") as fh:
        fh.write("tools/string_order_time.py on one MI355X (gfx950); the method of every figure is stated above its table\n\n" + text)


if __name__ == "__main__":
    main()
