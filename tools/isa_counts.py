"""Dev tool: instruction counts of one kernel in the compiled gfx950 assembly.

    python tools/isa_counts.py [kernel-substring] [extra hipcc flags...]

Compiles zelana_amd/csrc/msm.hip device-only to /tmp/zkmi_isa/msm.s (no GPU
needed) and prints, for the first kernel whose symbol contains the substring
(default k_acc_items_g1): VGPR / scratch / LDS metadata and the most frequent
instructions (e.g. v_mad_u64_u32 and the s_nop hazard fillers between
dependent mads), with the kernel's code size
(codeLenInByte) and its VALU, mad and s_nop counts on lines of their own.
ASM_FILE=path reads an assembly file made earlier instead of compiling."""
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
name = sys.argv[1] if len(sys.argv) > 1 else "k_acc_items_g1"
SRC = os.environ.get("SRC", "msm")
out = os.environ.get("ASM_FILE") or f"/tmp/zkmi_isa/{SRC}.s"
if not os.environ.get("ASM_FILE"):
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-w", "--cuda-device-only", "-S",
                    "-o", out, os.path.join(ROOT, "zelana_amd", "csrc", SRC + ".hip")] + sys.argv[2:], check=True)
s = open(out).read()
m = re.search(r"^(_Z[^\s:]*" + re.escape(name) + r"[^\s:]*):", s, re.M)
if not m:
    raise SystemExit(f"no kernel matching {name}")
i = m.start()
meta = s[i:s.index(".end_amdhsa_kernel", i)]
body = s[i:s.index(".Lfunc_end", i)]  # (the whole function: a kernel may hold s_endpgm more than once)
for key in (".amdhsa_next_free_vgpr", ".amdhsa_private_segment_fixed_size", ".amdhsa_group_segment_fixed_size"):
    k = re.search(re.escape(key) + r"\s+(\d+)", meta)
    print(f"{key:40s} {k.group(1) if k else '?'}")
lines = [l.strip() for l in body.splitlines()[1:]]
ins = [l.split()[0] for l in lines if l and not l.startswith((".", ";", "//")) and not l.endswith(":")]
k = re.search(r"codeLenInByte\s*=\s*(\d+)", s[i:])
print(f"{'codeLenInByte':40s} {k.group(1) if k else '?'}")
print(f"{'instructions':40s} {len(ins)}")
print(f"{'VALU (v_*)':40s} {sum(1 for o in ins if o.startswith('v_'))}")
print(f"{'v_mad_u64_u32':40s} {ins.count('v_mad_u64_u32')}")
print(f"{'s_nop':40s} {ins.count('s_nop')}")
for op, c in collections.Counter(ins).most_common(15):
    print(f"  {op:38s} {c}")
