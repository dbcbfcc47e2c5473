"""GPU idle time inside one product-embedding build, from the rocpd database of
`rocprofv3 --kernel-trace --stats -- python3 tools/embed_build_time.py N --build-only` (tools/embed_build_time.py runs a
warm-up build first: the timed build is what follows the longest pause, its filter_products).

    python tools/embed_trace_gaps.py <results.db>

Prints the span of the build's kernels, the time at least one kernel was running, the largest gaps, and how many
rr_wp_tokenize launches ran while an encoder kernel did (the tokenizer has a stream of its own)."""
import sqlite3
import sys

rows = sqlite3.connect(sys.argv[1]).execute("select start, end, name from kernels order by start").fetchall()
last_end, best, cut = rows[0][1], -1, 0
for i in range(1, len(rows)):
    if rows[i][0] - last_end > best:
        best, cut = rows[i][0] - last_end, i
    last_end = max(last_end, rows[i][1])
part = rows[cut:]
span = max(r[1] for r in part) - part[0][0]
busy, gaps, (s0, e0) = 0, [], part[0][:2]
for s, e, _ in part[1:]:
    if s > e0:
        busy += e0 - s0
        gaps.append(s - e0)
        s0, e0 = s, e
    else:
        e0 = max(e0, e)
busy += e0 - s0
gaps.sort(reverse=True)
enc = [(s, e) for s, e, n in part if "ce_" in n]
tok = [(s, e) for s, e, n in part if "rr_wp_tokenize" in n]
both = sum(any(s < fe and e > fs for fs, fe in enc) for s, e in tok)
print(f"pause before the timed build {best / 1e9:.3f} s; kernels {len(part)}; span {span / 1e9:.4f} s; busy {busy / 1e9:.4f} s; "
      f"idle {100 * (1 - busy / span):.2f} %")
print("largest gaps (us):", [round(g / 1e3) for g in gaps[:8]], "; gaps above 50 us:", sum(g > 50e3 for g in gaps))
print(f"rr_wp_tokenize launches that ran beside an encoder kernel: {both} of {len(tok)}")
