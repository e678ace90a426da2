#!/usr/bin/env bash
# Request counters of the shade kernels over the default bench command: what the vector L1 sends to the L2, what the L2
# sees, and the vector L1's busy share — each counter group in a rocprofv3 pass of its own, nothing but kernel tracing
# beside it — plus one --kernel-trace --stats pass.
#   usage: tools/profile_shade_records.sh <tag> [VAR=value ...]     (e.g. `before TAKE_HIP_SHADE_COOP=0`, `after`)
# writes $LOG_DIR/shade_records_<tag>/ (LOG_DIR: default bench_logs/, as the sweep scripts) and its summary
# shade_records_<tag>.txt beside it (tools/profile_shade_records.py; the curated copies are
# profiles/shade_records_<tag>.txt).  Counter names are checked against the GPU's own list (`rocprofv3 -L`, kept as
# counters_available.txt); a name it does not have is dropped from its pass and reported.
set -u
tag="$1"; shift
root="$(cd "$(dirname "$0")/.." && pwd)"
logs="${LOG_DIR:-$root/bench_logs}"
out="$logs/shade_records_$tag"; mkdir -p "$out"
export TMPDIR=/tmp; cd /tmp
for kv in "$@"; do export "$kv"; done
rocprofv3 -L > "$out/counters_available.txt" 2>&1
known() { local keep=(); for c in "$@"; do if grep -qw "$c" "$out/counters_available.txt"; then keep+=("$c"); else echo "counter $c: not in this GPU's counter list" >&2; fi; done; echo "${keep[@]}"; }
pass() {
    local name="$1"; shift
    local counters; counters=$(known "$@")
    [ -n "$counters" ] || { echo "pass $name: no counter left"; return 0; }
    # shellcheck disable=SC2086
    timeout -k 10 300 rocprofv3 --kernel-trace --pmc $counters --output-format csv -d "$out/$name" -- python3 "$root/bench.py" > "$out/$name.log" 2>&1
    local rc=$?; echo "pass $name ($counters) rc=$rc"; return $rc
}
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/stats" -- python3 "$root/bench.py" > "$out/stats.log" 2>&1 || { echo "stats pass failed"; exit 1; }
pass l1_l2 TCP_TCC_READ_REQ_sum TCP_TCC_WRITE_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum || exit 1
pass l2 TCC_REQ_sum TCC_HIT_sum TCC_MISS_sum || exit 1
pass l1_busy TCP_GATE_EN1_sum TCP_GATE_EN2_sum || exit 1
python3 "$root/tools/profile_shade_records.py" "$out" > "$logs/shade_records_$tag.txt" && cat "$logs/shade_records_$tag.txt"
