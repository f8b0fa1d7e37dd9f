#!/bin/bash
# A/B of library builds on one bench config: the variant libraries named in LIBS
# (miningsimulation_amd/variants/libmsim_NAME.so: `make -C miningsimulation_amd/csrc variant V=NAME VFLAGS=...`,
# or a copy of another commit's libmsim.so) alternate for REPS rounds, each on the default (two streams) and the
# serial line; with DUMP=1 the last step's outputs of every library are compared with the first one's, array for
# array. Every GPU step runs under its own timeout and the first failure ends the script.
#   CFG=c2 LIBS="parent new" REPS=3 MODES="0 1" DUMP=1 OUT=build/ab bash scripts/gpu_lib_ab.sh
set -o pipefail
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
CFG=${CFG:-c2}; LIBS=${LIBS:-"parent new"}; REPS=${REPS:-3}; MODES=${MODES:-"0 1"}
O=${OUT:-build/ab}_$CFG; mkdir -p $O
V=$PWD/miningsimulation_amd/variants
for i in $(seq 1 $REPS); do
  for L in $LIBS; do
    for s in $MODES; do
      MSIM_LIB=$V/libmsim_$L.so timeout -k 10 180 python3 bench.py --config $CFG --steps 40 --warmup 4 --streams $s > $O/${L}_s${s}_$i.json 2> $O/${L}_s${s}_$i.err || { tail -5 $O/${L}_s${s}_$i.err; exit 1; }
    done
  done
done
if [ -n "$DUMP" ]; then
  for L in $LIBS; do
    MSIM_LIB=$V/libmsim_$L.so timeout -k 10 180 python3 bench.py --config $CFG --steps 6 --warmup 1 --dump-outputs $O/dump_$L > $O/dump_$L.json 2> $O/dump_$L.err || { tail -5 $O/dump_$L.err; exit 1; }
  done
fi
python3 - <<EOF
import json, glob, os
O = "$O"
rows = {}
for f in sorted(glob.glob(O + "/*_s[01]_*.json")):
    lib, s, i = os.path.basename(f)[:-5].rsplit("_", 2)
    d = json.loads(open(f).read().strip().splitlines()[-1])
    rows.setdefault((lib, s), []).append((d["value"], d["ms_per_step"], d["roofline"]["dominant_ms"]))
for (lib, s), v in sorted(rows.items(), key=lambda kv: (kv[0][1], kv[0][0])):
    vals = [x[0] for x in v]
    print(f"$CFG {lib:10s} {s}  run-years/s {min(vals):.0f} .. {max(vals):.0f}  mean {sum(vals)/len(vals):.0f}  ms/step "
          + " ".join(f"{x[1]:.3f}" for x in v) + "  dominant_ms " + " ".join(f"{x[2]:.3f}" for x in v))
libs = "$LIBS".split()
if "$DUMP":
    import numpy as np
    a = libs[0]
    for b in libs[1:]:
        for name in ("sums_words", "sums", "status"):
            x, y = np.load(f"{O}/dump_{a}/{name}.npy"), np.load(f"{O}/dump_{b}/{name}.npy")
            print(f"$CFG dump {a} vs {b} {name}: {'EQUAL' if x.shape == y.shape and np.array_equal(x, y) else 'DIFFERENT'} {x.shape}")
EOF
