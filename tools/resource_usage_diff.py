"""Compare the kernel-resource-usage remarks of two `python -m text2speech_amd.build --force -v` logs (stderr), kernel by kernel.

    python -m text2speech_amd.build --force -v 2> before.log      # on the parent commit
    python -m text2speech_amd.build --force -v 2> after.log
    python tools/resource_usage_diff.py before.log after.log > profiles/NAME.md

Kernels are matched by demangled name.  A kernel that gained template parameters with defaults shows them in its mangled name, so
the operand-format parameters (`T2sFmtBf16`, and the `false` behind it where the kernel also has the one-plane switch) are
dropped from the "after" names before matching, as is the ping-pong gate kernel's `RAG` parameter where it is `false`; what is left
unmatched on the "after" side is listed as new.
"""
import re
import subprocess
import sys

FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]"]


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        body = m.group(1).strip()
        if body.startswith("Function Name:"):
            cur = body.split(":", 1)[1].strip()
            out[cur] = {}
        elif cur is not None and ":" in body:
            k, v = body.rsplit(":", 1)
            out[cur][k.strip()] = v.strip()
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def normalise(name):
    name = re.sub(r"^void ", "", name)
    # gate_gemm_pp_kernel's fifth parameter (RAG, default false) came after the format parameters: drop it where it is false
    name = re.sub(r"^(gate_gemm_pp_kernel<[^,<>]+, [^,<>]+, [^,<>]+, [^,<>]+), false>", r"\1>", name)
    for pat, rep in ((", T2sFmtBf16, false>", ">"), ("<T2sFmtBf16, false>", ""), (", T2sFmtBf16>", ">"), ("<T2sFmtBf16>", "")):
        name = name.replace(pat, rep)
    return name


def main():
    before, after = parse(sys.argv[1]), parse(sys.argv[2])
    db, da = demangle(list(before)), demangle(list(after))
    b = {normalise(db[k]): v for k, v in before.items()}
    a = {normalise(da[k]): v for k, v in after.items()}
    changed, same, gone = [], 0, []
    for name, rb in sorted(b.items()):
        ra = a.get(name)
        if ra is None:
            gone.append(name)
        elif any(rb.get(f) != ra.get(f) for f in FIELDS):
            changed.append((name, rb, ra))
        else:
            same += 1
    new = sorted(n for n in a if n not in b)
    print("| | count |\n|---|---|")
    print("| kernels before | %d |\n| unchanged in every field (%s) | %d |\n| changed | %d |\n| missing after | %d |\n| new | %d |"
          % (len(b), ", ".join(FIELDS), same, len(changed), len(gone), len(new)))
    for name, rb, ra in changed:
        print("\nCHANGED `%s`" % name)
        for f in FIELDS:
            if rb.get(f) != ra.get(f):
                print("- %s: %s -> %s" % (f, rb.get(f), ra.get(f)))
    for name in gone:
        print("\nMISSING `%s`" % name)
    if new:
        print("\nNew kernels:\n\n| kernel | " + " | ".join(FIELDS) + " |\n|---|" + "---|" * len(FIELDS))
        for name in new:
            print("| `%s` | " % name + " | ".join(a[name].get(f, "") for f in FIELDS) + " |")
    return 1 if changed or gone else 0


if __name__ == "__main__":
    sys.exit(main())
