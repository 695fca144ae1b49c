"""Register and scratch use of every kernel of the product build (the compiler's own report,
-Rpass-analysis=kernel-resource-usage, on the Makefile's flags), one line per kernel.

    python3 tools/resource_report.py > profiles/spectator_resource_usage.txt

A p2p_kernel instantiation is printed with its variant's flags by name (p2p_variant.hpp P2PFlag),
p2p_kernel<ExGame<2, true>, LdsC|Async|Log>.  With --against REPORT (a report of another commit,
made the same way) every kernel line of a translation unit the other report lists is followed by
how it compares with that report; a p2p_kernel line compares with the instantiation of
the same flags there; a report from when the flags were ten positional bool template arguments
(missing trailing ones false) is read as the same names.  Instantiations only the other report has
are listed at the end.

    python3 tools/resource_report.py --against parent_report.txt ops_exgame_p2.hip ...

profiles/time_sync_resource_usage.txt was made that way against
profiles/time_sync_resource_usage_parent.txt, this tool's report of the commit before it.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ggrs_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-DRB_EXPERIMENTS=0"]
AGAINST = None
if "--against" in sys.argv:
    i = sys.argv.index("--against")
    AGAINST = sys.argv[i + 1]
    del sys.argv[i:i + 2]
P2P_FLAGS = ["Spec", "Sparse", "Net", "LdsC", "Async", "Wire", "Mtf", "Q", "One", "Log"]  # bit 0 .. 9, the old argument order
TUS = sys.argv[1:] or ["ops_exgame_p2.hip", "ops_exgame_p3.hip", "ops_exgame_p4.hip", "ops_brawler_p2.hip", "ops_stub.hip"]


def p2p_name(n):
    """p2p_kernel<G, 24u> or p2p_kernel<G, false, false, false, true, true> as p2p_kernel<G, LdsC|Async>."""
    m = re.fullmatch(r"(p2p_kernel<.*?), (\d+)u>", n) or re.fullmatch(r"(p2p_kernel<.*?)((?:, (?:true|false))+)>", n)
    if not m:
        return n
    on = ([(int(m.group(2)) >> i) & 1 for i in range(len(P2P_FLAGS))] if m.group(2).isdigit()
          else [a == "true" for a in m.group(2)[2:].split(", ")])
    return f"{m.group(1)}, {'|'.join(f for f, b in zip(P2P_FLAGS, on) if b) or '0'}>"


def load_report(path):
    """{(translation unit, kernel): the eight numbers} of a report this tool wrote."""
    out, tu = {}, None
    for line in open(path):
        if line.startswith("## "):
            tu = line[3:].strip()
        elif line.strip() and not line.startswith("#"):
            f = line.split(None, 8)
            out[tu, p2p_name(f[8].split("   [")[0].strip())] = tuple(int(x) for x in f[:8])
    return out


def main():
    base = load_report(AGAINST) if AGAINST else None
    same = changed = added = 0
    other = [0, 0, 0]  # the kernels that are no p2p_kernel, where the other report lists their translation unit: same, changed, new
    print(f"# {' '.join(FLAGS)} (+ -mllvm -amdgpu-sched-strategy=max-ilp for ops_exgame_p*, as the Makefile)")
    print(f"# {'VGPR':>4s} {'AGPR':>4s} {'SGPR':>4s} {'SGPR spill':>10s} {'VGPR spill':>10s} {'scratch B/lane':>14s} "
          f"{'waves/SIMD':>10s} {'LDS B':>6s}  kernel")
    listed = []
    for tu in TUS:
        extra = ["-mllvm", "-amdgpu-sched-strategy=max-ilp"] if tu.startswith("ops_exgame_p") else []
        with tempfile.TemporaryDirectory() as td:
            p = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + extra + ["--cuda-device-only", "-S", "-o",
                               os.path.join(td, "x.s"), tu, "-Rpass-analysis=kernel-resource-usage"],
                               cwd=CSRC, capture_output=True, text=True)
        rows, cur = [], None
        for line in p.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = {"name": m.group(1)}
                rows.append(cur)
                continue
            for key, tag in (("VGPRs: ", "v"), ("AGPRs: ", "a"), ("SGPRs: ", "s"), ("SGPRs Spill: ", "ss"),
                             ("VGPRs Spill: ", "vs"), ("ScratchSize [bytes/lane]: ", "sc"),
                             ("Occupancy [waves/SIMD]: ", "o"), ("LDS Size [bytes/block]: ", "l")):
                m = re.search(re.escape(key) + r"(\d+)", line)
                if m and cur is not None:
                    cur[tag] = int(m.group(1))
        print(f"## {tu}")
        for r in rows:
            n = subprocess.run(["c++filt", r["name"]], capture_output=True, text=True).stdout.strip()
            if "kernel" not in n:
                continue
            n = n.replace("(anonymous namespace)::", "")
            n = n[5:] if n.startswith("void ") else n
            n = n.replace("rb::", "")
            n = p2p_name(n.split("(")[0])
            vals = tuple(r.get(k, 0) for k in ("v", "a", "s", "ss", "vs", "sc", "o", "l"))
            note = ""
            if base is not None and n.startswith("p2p_kernel<"):
                old = base.pop((tu, n), None)
                if old is None:
                    added += 1
                    note = "   [new]"
                elif old == vals:
                    same += 1
                    note = "   [= parent]"
                else:
                    changed += 1
                    note = f"   [CHANGED, parent: {' '.join(map(str, old))}]"
            elif base is not None and any(k[0] == tu for k in list(base) + listed):
                old = base.pop((tu, n), None)
                listed.append((tu, n))
                other[0 if old == vals else 2 if old is None else 1] += 1
                note = ("   [= parent]" if old == vals else "   [new]" if old is None
                        else f"   [CHANGED, parent: {' '.join(map(str, old))}]")
            print(f"  {vals[0]:4d} {vals[1]:4d} {vals[2]:4d} {vals[3]:10d} {vals[4]:10d} "
                  f"{vals[5]:14d} {vals[6]:10d} {vals[7]:6d}  {n}{note}")
    if base is not None:
        gone = sorted(k for k in base if k[0] in TUS and k[1].startswith("p2p_kernel<"))
        for tu, n in gone:
            print(f"# only in {os.path.basename(AGAINST)}: {tu} {n}")
        print(f"# p2p_kernel instantiations against {os.path.basename(AGAINST)}: {same} unchanged, {changed} changed, "
              f"{added} new" + (f", {len(gone)} GONE" if gone else ""))
        lost = sorted(k for k in base if k[0] in TUS and not k[1].startswith("p2p_kernel<"))
        for tu, n in lost:
            print(f"# only in {os.path.basename(AGAINST)}: {tu} {n}")
        print(f"# other kernels (codec, liveness, engines) against {os.path.basename(AGAINST)}: {other[0]} unchanged, "
              f"{other[1]} changed, {other[2]} new" + (f", {len(lost)} GONE" if lost else ""))


if __name__ == "__main__":
    main()
