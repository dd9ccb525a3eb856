#!/bin/bash
# GPU box helper: run ONE step under its own time limit; stop the whole call on
# a timeout, a signal or a crash (status >= 124), keep going after an ordinary
# failure (a failed assertion) so the later steps still report.
# usage: source tools/gpu_step.sh; step NAME SECONDS cmd args...   (output: $OUT/NAME.log, OUT defaults to bench_out)
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
step() {
	local name=$1 secs=$2
	shift 2
	echo "== $name: $*"
	timeout -k 10 "$secs" "$@" > "$OUT/$name.log" 2>&1
	local rc=$?
	tail -3 "$OUT/$name.log"
	echo "== $name rc=$rc"
	if [ $rc -ge 124 ]; then
		echo "abnormal exit ($rc): stopping"
		exit $rc
	fi
	return 0
}
