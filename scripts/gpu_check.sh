# quick GPU regression: parity suite, latency probe, batch bench (used during development)
cd $GRAFT_REPO_ROOT
OUT=${CHECK_OUT:-$(mktemp -d)}  # where the bench line is kept
mkdir -p "$OUT"
timeout 1200 python -m pytest tests -m gpu -x -q 2>&1 | tail -25
timeout 300 python scripts/latency_probe.py 2>&1 | tail -3
timeout 300 python bench.py --full --no-cpu-baseline > "$OUT/bench.json" 2>&1; tail -1 "$OUT/bench.json" | cut -c1-200
