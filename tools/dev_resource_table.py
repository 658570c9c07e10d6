"""Kernel resource usage as a table, from the compiler's remarks.

    python -m smarts_amd.build --force 2> remarks.txt        # (-Rpass-analysis=kernel-resource-usage)
    python tools/dev_resource_table.py remarks.txt [FILTER ...]

One line per kernel: VGPRs, AGPRs, SGPRs, scratch bytes per lane, LDS bytes per workgroup, wavefronts per SIMD, and
the demangled name (template arguments kept: a trailing `false` / `true` is the GUARD parameter of the control, reset
and tail kernels).  FILTER: keep kernels whose name contains one of the words.  With --compare OTHER.txt the kernels of
OTHER whose name, less a trailing `, false` / `<false>` argument, equals one here are put beside them and every
difference is marked.  profiles/r12_guard_resources.txt was made with it.  With --same-names as well the kernels are
paired by their full names (both builds have the same kernels: profiles/r16_traffic_history_resources.txt).
"""
import re
import subprocess
import sys

KEYS = [("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("TotalSGPRs", "SGPRs"), ("ScratchSize [bytes/lane]", "scratch"),
        ("LDS Size [bytes/block]", "LDS"), ("Occupancy [waves/SIMD]", "waves")]


def parse(path):
    kernels, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+): (\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    names = list(kernels)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    out = {}
    for mangled, name in zip(names, dem):
        name = re.sub(r"^void ", "", name)
        name = re.sub(r"\(.*\)$", "", name)
        out[name] = tuple(kernels[mangled].get(k, "?") for k, _ in KEYS)
    return out


GUARDED = ("k_control", "k_reset<", "k_tail<")  # the kernels whose last template argument is GUARD


def guarded(name):
    return name.startswith(GUARDED)


def base(name):
    """The name with a trailing GUARD = false argument dropped (the parent's kernels have no such parameter)."""
    if not guarded(name):
        return name
    name = re.sub(r", false>$", ">", name)
    return re.sub(r"<false>$", "", name)


def main(argv):
    compare = None
    same_names = "--same-names" in argv
    argv = [a for a in argv if a != "--same-names"]
    if "--compare" in argv:
        i = argv.index("--compare")
        compare = parse(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    table = parse(argv[0])
    words = argv[1:]
    head = "".join(f"{short:>8}" for _, short in KEYS)
    print(head + ("   |" + head if compare else "") + "   kernel")
    differ = 0
    for name in sorted(table):
        if words and not any(w in name for w in words):
            continue
        row = "".join(f"{v:>8}" for v in table[name])
        if compare is None:
            print(row + "   " + name)
            continue
        if not same_names and guarded(name) and name.endswith("true>"):
            print(row + "   |" + " " * len(head) + "   " + name)
            continue
        other = compare.get(name if same_names else base(name))
        if other is None:
            print(row + "   |" + f"{'(absent)':>{len(head)}}" + "   " + name)
            continue
        mark = "" if other == table[name] else "   <-- DIFFERS"
        differ += bool(mark)
        print(row + "   |" + "".join(f"{v:>8}" for v in other) + "   " + name + mark)
    if compare is not None:
        print(f"# kernels that differ from their namesake: {differ}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
