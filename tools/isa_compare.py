"""Compare the gfx950 kernels of two builds of libemei_hip.so, symbol by symbol: the stream of (mnemonic, operands) that
llvm-objdump -d prints for each function of the bundled code objects (addresses and encodings dropped).

    python tools/isa_compare.py OLD.so NEW.so [--only REGEX]

Prints how many symbols are identical, lists the ones that differ (with the first differing instruction) and the ones only one side
has, and exits 1 when a symbol both sides have differs.  For a change that must leave existing kernels as they are."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
_INS = re.compile(r"^\s+(\S+)\s*(.*?)\s*//\s*[0-9A-Fa-f]+:")


def functions(lib):
    """{mangled name: [(mnemonic, operands)]} over every gfx950 code object bundled in `lib`"""
    funcs = {}
    with tempfile.TemporaryDirectory() as d:
        copy = shutil.copy(lib, d)
        subprocess.check_call([OBJDUMP, "--offloading", copy], stdout=subprocess.DEVNULL, cwd=d)
        for f in sorted(os.listdir(d)):
            if "gfx950" not in f:
                continue
            cur = None
            for line in subprocess.check_output([OBJDUMP, "-d", os.path.join(d, f)], text=True).splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    cur = funcs.setdefault(m.group(1), [])
                    continue
                m = _INS.match(line)
                if m and cur is not None:
                    cur.append((m.group(1), m.group(2)))
    return funcs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--only", default=".", help="regex on the mangled name")
    a = ap.parse_args()
    old, new = functions(a.old), functions(a.new)
    pick = re.compile(a.only)
    both = sorted(k for k in old if k in new and pick.search(k))
    differ = [k for k in both if old[k] != new[k]]
    print(f"{len(both)} symbols in both, {len(both) - len(differ)} identical, {len(differ)} differ")
    for k in differ:
        at = next((j for j, (x, y) in enumerate(zip(old[k], new[k])) if x != y), min(len(old[k]), len(new[k])))
        print(f"  DIFFERS {k}: {len(old[k])} -> {len(new[k])} instructions, first at #{at}: "
              f"{old[k][at] if at < len(old[k]) else None} -> {new[k][at] if at < len(new[k]) else None}")
    for side, xs, ys in (("old", old, new), ("new", new, old)):
        only = sorted(k for k in xs if k not in ys and pick.search(k))
        print(f"only in {side}: {len(only)}")
        for k in only:
            print(f"  {k}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
