"""Static instruction count of one kernel in a `make asm` listing (needs no GPU).

    make -C ggrs_amd/csrc asm
    python3 tools/asm_count.py ggrs_amd/csrc/build/ops_exgame_p2-gfx950.s 'steady_kernel<rb::ExGame<2, true>, 7, false>'

(`make asm` compiles without the Makefile's per-unit TU_FLAGS; for ops_exgame_p* add
`-mllvm -amdgpu-sched-strategy=max-ilp` by hand to get the product's schedule.)  Prints, for
every function whose demangled name contains the given text, the lines whose mnemonic starts
with v_ (VALU), with s_ (SALU, waits and branches included), the memory instructions, and the
most frequent VALU mnemonics.
"""
import collections
import re
import subprocess
import sys


def main():
    path, want = sys.argv[1], sys.argv[2]
    top = int(sys.argv[3]) if len(sys.argv) > 3 else 12
    name, body, funcs = None, [], []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name and line.startswith("\t.end_amdhsa_kernel"):
            name = None
        if name and line.startswith("\ts_endpgm"):
            body.append(line)
            funcs.append((name, body))
            name = None
            continue
        if name:
            body.append(line)
    for name, body in funcs:
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        if want not in dem:
            continue
        ops = [l.split()[0] for l in body if re.match(r"^\t[a-z]", l) and not l.startswith("\t.")]
        valu = [o for o in ops if o.startswith("v_")]
        salu = [o for o in ops if o.startswith("s_")]
        mem = [o for o in ops if o.split("_")[0] in ("global", "flat", "buffer", "scratch", "ds")]
        print(f"{dem}\n  VALU {len(valu)}  SALU {len(salu)}  memory {len(mem)}  all {len(ops)}")
        for o, n in collections.Counter(valu).most_common(top):
            print(f"    {n:5d} {o}")


if __name__ == "__main__":
    main()
