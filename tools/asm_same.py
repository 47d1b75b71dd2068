#!/usr/bin/env python3
"""Compare the kernels of two device assembly files (hipcc ... --cuda-device-only -S), symbol by symbol:
    tools/asm_same.py [--map OLD=NEW]... parent.s new.s
A kernel is SAME when the text between its label and its .Lfunc_end label and its .amdhsa_kernel block are identical.  Block labels, and
the comments that name them, carry the function's ordinal in the file (BB<fn>_<n>), which moves when a kernel is added in front of
it: the ordinal is dropped before the comparison, and with it the padding in front of a label's comment.
--map (repeatable) renames on the parent side before the comparison: every occurrence of OLD, a substring of a symbol, becomes NEW."""
import re
import sys


def kernels(path, maps=()):
    s = open(path).read()
    for old, new in maps:
        s = s.replace(old, new)
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", s, re.M | re.S):
        name, hsa = m.group(1), m.group(2)
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), s, re.M | re.S).group(1)
        body = re.sub(r"[ \t]+;", " ;", re.sub(r"BB\d+_(\d+)", r"BB_\1", body))
        num = {k: int(re.search(r"\.amdhsa_%s (\d+)" % k, hsa).group(1))
               for k in ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")}
        out[name] = (body, hsa, num)
    return out


args, maps = sys.argv[1:], []
while "--map" in args:
    i = args.index("--map")
    maps.append(tuple(args[i + 1].split("=", 1)))
    del args[i:i + 2]
a, b = kernels(args[0], maps), kernels(args[1])
print(f"{'':4} {'lines':>6} {'vgpr':>5} {'sgpr':>5} {'scratch':>7} {'lds':>7}  kernel")
for name in sorted(set(a) | set(b)):
    same = name in a and name in b and a[name][:2] == b[name][:2]
    body, _, n = (b if name in b else a)[name]
    print(f"{'SAME' if same else 'DIFF'} {body.count(chr(10)):6d} {n['next_free_vgpr']:5d} {n['next_free_sgpr']:5d} "
          f"{n['private_segment_fixed_size']:7d} {n['group_segment_fixed_size']:7d}  {name}")
print(f"{sum(n in b and a[n][:2] == b[n][:2] for n in a)} of {len(set(a) | set(b))} kernels identical")
