"""Developer: timeline of one forked tick from a rocprofv3 --kernel-trace CSV (kernel_trace.csv).
    python tools/dev_timeline.py <kernel_trace.csv> [tick index from the end, default 3]
A tick starts with its first kernel: k_social, k_alive_list or the controller, whichever comes first (the alive list
is usually built by the last tick's k_tail, and k_alive_list then does not run)."""
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
k = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].replace("void ", ""), r.get("Stream_Id", r.get("Queue_Id", "?"))) for r in rows]
k.sort()
HEAD = ("k_social", "k_alive_list", "k_control")
starts = [i for i, r in enumerate(k) if r[2].startswith(HEAD) and (i == 0 or not k[i - 1][2].startswith(HEAD))]
which = int(sys.argv[2]) if len(sys.argv) > 2 else 3
a = starts[-which - 1]; b = starts[-which]
t0 = k[a][0]
print(f"tick of {(k[b][0] - t0) / 1e3:.1f} us (first kernel to first kernel)")
for s, e, name, q in k[a:b]:
    print(f"{(s - t0) / 1e3:8.1f} -> {(e - t0) / 1e3:8.1f}  ({(e - s) / 1e3:7.1f})  q{q:>3s}  {name}")
# average tick over the last 20 (or as many as the trace holds)
n = min(20, len(starts) - 1)
d = [(k[starts[i + 1]][0] - k[starts[i]][0]) / 1e3 for i in range(len(starts) - 1 - n, len(starts) - 1)]
print("mean of the last %d ticks: %.1f us" % (n, sum(d) / len(d)))
