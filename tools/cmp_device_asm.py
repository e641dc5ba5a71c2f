"""Compare the gfx950 code of every kernel in one device listing against the same kernels spread over other listings (after moving
kernels between source files).  Listings: hipcc <the Makefile's flags> --cuda-device-only -S file.hip -o file.s
usage: cmp_device_asm.py old.s new1.s [new2.s ...]   -> a markdown table; exit status 1 if a kernel is missing, doubled or differs"""
import re
import sys

RES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    """{kernel symbol: (resource block, normalised instruction lines)}"""
    s = open(path).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", s, re.S):
        name = m.group(1)
        res = tuple(re.search(r"\.amdhsa_%s (\S+)" % r, m.group(2)).group(1) for r in RES)
        body = s[s.index("\n%s:" % name):].split("s_endpgm")[0].split("\n")[2:]
        code = []
        for l in body:
            l = re.sub(r"(\.L[A-Za-z_]+)\d+_", r"\1_", l.split(";")[0]).strip()   # comments off, function number out of local labels
            if l and not re.match(r"\.(loc|file|cfi_)", l):
                code.append(l)
        out[name] = (res, code)
    return out


old = kernels(sys.argv[1])
new = {}
for p in sys.argv[2:]:
    for k, v in kernels(p).items():
        new.setdefault(k, []).append((p.split("/")[-1], v))
bad = 0
print("| kernel | listing | VGPRs | scratch bytes | instructions | same |\n|---|---|---|---|---|---|")
for k in sorted(old):
    res, code = old[k]
    n_ins = sum(1 for l in code if not l.startswith(".") and not l.endswith(":"))
    homes = new.get(k, [])
    if len(homes) != 1:
        verdict = "MISSING" if not homes else "IN %d LISTINGS" % len(homes)
    else:
        verdict = "same" if homes[0][1] == (res, code) else "DIFFERS (resources %s)" % ("same" if homes[0][1][0] == res else homes[0][1][0])
    bad += verdict != "same"
    print("| `%s` | %s | %s | %s | %d | %s |" % (k, homes[0][0] if homes else "-", res[0], res[4], n_ins, verdict))
extra = sorted(set(new) - set(old))
for k in extra:
    print("| `%s` | %s | | | | NOT IN %s |" % (k, new[k][0][0], sys.argv[1].split("/")[-1]))
print("\n%d kernels, %d not the same, %d new" % (len(old), bad, len(extra)))
sys.exit(1 if bad or extra else 0)
