"""Compare the device code of the working tree with that of another revision.

    python tools/device_code_diff.py REV

REV is checked out into a temporary directory (``git archive``).  Every ``csrc/*.hip`` of that
tree and of the working tree is compiled to device-only assembly with the build's flags
(``csrc/build.py``: the common ones plus ``PER_FILE_FLAGS``) and ``--cuda-device-only -S``, once
without and once with ``-DPIO_CHECKS=1``.  The per-compilation ``__hip_cuid_<hex>`` symbol is
blanked out, then the two texts must be equal.  Prints one line per file and variant
("identical", or the first differing lines) and exits non-zero on any difference.  A change
that touches only host code (launchers, the binding, shared host headers) must pass.

Jobs: ``MAX_JOBS`` (default 16).
"""
from __future__ import annotations

import difflib
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from perceiver_io_amd.csrc.build import HIP_FLAGS, HIPCC, PER_FILE_FLAGS  # noqa: E402

CSRC = Path("perceiver_io_amd") / "csrc"
VARIANTS = {"release": [], "checked": ["-DPIO_CHECKS=1"]}
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")


def device_asm(src: Path, extra, out: Path) -> str:
    cmd = [HIPCC, *HIP_FLAGS, "-O3", *extra, *PER_FILE_FLAGS.get(src.name, []), "-I", str(src.parent),
           "--cuda-device-only", "-S", str(src), "-o", str(out)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(" ".join(cmd) + "\n" + r.stdout)
    return CUID.sub("__hip_cuid_", out.read_text())


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1:
        print(__doc__)
        return 2
    rev = argv[0]
    jobs = int(os.environ.get("MAX_JOBS", 16))
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        old = tmp / "old"
        old.mkdir()
        tar = tmp / "rev.tar"
        subprocess.run(["git", "-C", str(ROOT), "archive", "-o", str(tar), rev, str(CSRC)], check=True)
        with tarfile.open(tar) as t:
            t.extractall(old)
        names = sorted({p.name for tree in (old, ROOT) for p in (tree / CSRC).glob("*.hip")})
        work = [(n, v) for n in names for v in VARIANTS]

        def one(item):
            name, variant = item
            texts = []
            for tag, tree in (("old", old), ("new", ROOT)):
                src = tree / CSRC / name
                if not src.exists():
                    return name, variant, [f"missing in the {'revision' if tag == 'old' else 'working tree'}"]
                texts.append(device_asm(src, VARIANTS[variant], tmp / f"{tag}.{variant}.{name}.s"))
            if texts[0] == texts[1]:
                return name, variant, None
            d = difflib.unified_diff(texts[0].splitlines(), texts[1].splitlines(), rev, "working tree", lineterm="", n=1)
            return name, variant, [ln for _, ln in zip(range(20), d)]

        with ThreadPoolExecutor(max_workers=jobs) as ex:
            results = list(ex.map(one, work))
    bad = 0
    for name, variant, diff in results:
        print(f"{name:20s} {variant:8s} {'identical' if diff is None else 'DIFFERS'}")
        if diff is not None:
            bad += 1
            print("\n".join("    " + ln for ln in diff))
    print(f"{len(results) - bad} of {len(results)} identical ({len(names)} translation units x {len(VARIANTS)} variants)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
