#!/usr/bin/env python3
"""Same-box A/B of the default bench command between two builds of libfdtd_hip.so and the traffic switches of this one.

    python3 tools/bench_ab.py <directory with the parent's libfdtd_hip.so> [runs per variant = 5] [out.jsonl]

Runs `python3 bench.py --gpus 1 --steps 20 --warmup 5` alternating: parent library ($FDTD_HIP_LIB_DIR), this build, this build with
$FDTD_CLASS_ROWS=0 (inert psi indices skipped, per-cell class bytes) and with $FDTD_PSI_ACTIVE=0 (class rows, psi ranges untrimmed).
Prints every `value` / `ms_per_step`, the medians and min-to-max spreads, and for each variant whether its median differs from the
parent's by more than twice the larger of the two spreads — the bar profiles/cpml_bytes/README.md uses.  Each run is a process of its
own under a time limit; the first failure ends the series."""
import json
import os
import statistics as st
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [("parent", None), ("A+B", {}), ("A_only", {"FDTD_CLASS_ROWS": "0"}), ("B_only", {"FDTD_PSI_ACTIVE": "0"})]


def main():
    parent = os.path.abspath(sys.argv[1])
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out = open(sys.argv[3], "w") if len(sys.argv) > 3 else None
    assert os.path.isfile(os.path.join(parent, "libfdtd_hip.so")), parent
    got = {name: [] for name, _ in VARIANTS}
    for _ in range(runs):
        for name, env in VARIANTS:
            e = dict(os.environ)
            e.update({"FDTD_HIP_LIB_DIR": parent} if env is None else env)
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                               env=e, cwd=ROOT, capture_output=True, text=True, timeout=300)
            lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not lines:
                sys.stderr.write(r.stderr[-2000:])
                raise SystemExit(f"bench.py failed for {name} (rc {r.returncode})")
            d = json.loads(lines[-1])
            got[name].append((d["value"], d["ms_per_step"]))
            print(name, d["value"], d["ms_per_step"], flush=True)
            if out:
                out.write(json.dumps({"variant": name, "line": d}) + "\n"); out.flush()
    p = [v for v, _ in got["parent"]]
    for name, rows in got.items():
        v, ms = [a for a, _ in rows], [b for _, b in rows]
        print(f"{name:7s} value median {st.median(v):.1f} (min-to-max {max(v) - min(v):.1f})  ms_per_step median {st.median(ms):.4f} (min-to-max {max(ms) - min(ms):.4f})")
    for name, rows in got.items():
        if name == "parent":
            continue
        v = [a for a, _ in rows]
        d, bar = st.median(v) - st.median(p), 2 * max(max(v) - min(v), max(p) - min(p))
        print(f"{name}: median {d:+.1f} Mcells/s ({100 * d / st.median(p):+.2f} %) against the parent; bar {bar:.1f}: {'gain' if d > bar else 'no gain'}")


if __name__ == "__main__":
    main()
