"""Writes tests/golden/program_images.json: the image (tests/program_images.py) of every case there.  Run at the commit a
rewrite of the lowerings starts from, never from the rewritten code: tests/test_program_images.py then proves that the rewrite
changes no byte the device receives.  The file records the commit it was written from (pass it as the first argument)."""
from __future__ import annotations

import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE), HERE):
    sys.path.insert(0, p)

import program_images  # noqa: E402


def main() -> None:
    out = {"#recorded_from": sys.argv[1] if len(sys.argv) > 1 else "unknown"}
    for name, run in program_images.cases().items():
        t0 = time.perf_counter()
        out[name] = run()
        print(f"{time.perf_counter() - t0:6.1f} s  {name}", flush=True)
    with open(os.path.join(HERE, "program_images.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
