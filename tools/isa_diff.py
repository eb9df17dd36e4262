"""Compare the gfx950 machine code of the same kernels in two builds of a library (no GPU): the
check a refactor of a kernel file needs -- every surviving kernel instantiation must come out
instruction for instruction as before.

  python tools/isa_diff.py OLD.so NEW.so PATTERN [--rename REGEX=REPL ...] [--show N]

Both libraries' device code is extracted and disassembled with llvm-objdump (as
tests/test_isa_lds_reads.py does), kernel names are demangled (llvm-objdump -C), and every kernel of NEW whose name
matches PATTERN (a regex on the demangled name without its parameter list) is compared with the
kernel of the same name in OLD. --rename rewrites OLD's names first, for kernels whose template
list changed, e.g. --rename 'attn_fwd_k<(\\d+), (\\w+), 4, 0>=attn_fwd_k<\\1, \\2>'. Addresses
(the pc-relative distance to a global variable included), encodings and symbol annotations are
stripped; what is compared is the instruction text, branch offsets included. Prints one line per kernel (identical yes / NO with the first differing
instructions), the OLD-only and NEW-only names matching PATTERN, and exits 1 on any difference
or any NEW kernel without a partner.
"""
import argparse
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def kernels(lib):
    """{demangled name without parameters: [instruction text]} of every gfx950 function in lib"""
    tmp = tempfile.mkdtemp()
    try:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(lib, so)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", so], cwd=tmp, check=True, capture_output=True)
        out = {}
        for f in sorted(os.listdir(tmp)):
            if not f.endswith("gfx950"):
                continue
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "-C", os.path.join(tmp, f)], check=True,
                                 capture_output=True, text=True).stdout
            name, getpc = None, -9
            for line in dis.split("\n"):
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    d = re.sub(r"^void ", "", m.group(1)).replace("(anonymous namespace)::", "")
                    name = d[:d.index(">(") + 1] if ">(" in d else d.split("(")[0]
                    out[name] = []
                elif name and line.startswith("\t") and line.strip() != "...":
                    ins = " ".join(re.sub(r"<[^>]*>", "", line.split("//")[0]).split())
                    # the pc-relative address of a global (s_getpc_b64, then s_add_u32 / s_addc_u32 with
                    # the distance as a literal) moves with the library's layout: an address, masked
                    if ins.startswith("s_getpc_b64"):
                        getpc = len(out[name])
                    elif len(out[name]) - getpc <= 2 and ins.startswith(("s_add_u32", "s_addc_u32")):
                        ins = re.sub(r"0x[0-9a-f]+$", "PCREL", ins)
                    out[name].append(ins)
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("pattern")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL")
    ap.add_argument("--show", type=int, default=6, help="differing lines printed per kernel")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    for r in a.rename:
        rx, repl = r.split("=", 1)
        old = {re.sub(rx, repl, n): body for n, body in old.items()}
    pat = re.compile(a.pattern)
    bad = 0
    for n in sorted(k for k in new if pat.search(k)):
        if n not in old:
            print(f"NEW ONLY   {n}")
            bad += 1
            continue
        same = old[n] == new[n]
        print(f"identical {'yes' if same else 'NO '} {len(new[n]):6d} instructions  {n}")
        if not same:
            bad += 1
            diff = [d for d in difflib.unified_diff(old[n], new[n], "old", "new", lineterm="", n=0)][2:]
            for d in diff[:a.show]:
                print("    " + d)
    for n in sorted(k for k in old if pat.search(k) and k not in new):
        print(f"old only   {n}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
