#!/bin/bash
# Would the vertical bilateral verdicts pay for themselves inside the top-hat walks?  The gate of that fusion, measured before
# building it: variant builds (results WRONG, timing only) through bench.py's one-stream pass, 256 frames per launch,
# rocprofv3 --kernel-trace --stats, the variants in turn, two rounds:
#   base   the library as it is
#   vsum   the 55x55 / 29x29 top-hat walks hold a register ring of top-hat dwords and issue the vertical pass's VALU work
#          (running sums, half-wave exchange, bias-folded verdicts, v_cmp) -- k_tophat_vsum.patch, -DLT_PROBE_VSUM
#   ring   the ring alone: its registers and its indexed moves, no sums (-DLT_PROBE_VSUM_RING_ONLY)
#   walkh  k_bilateral_walk_hv without its vertical tasks -- k_threshold_walk_honly.patch, -DLT_PROBE_WALK_H_ONLY
# then one PMC pass per counter group for base and vsum.      bash tools/fuse_gate.sh        (on the GPU box, from the repo root)
# the probe blocks live in tools/probes/*.patch, not in the product sources: patched copies of the two files are compiled here
set -u
root=$(pwd)
out=${FUSE_GATE_OUT:-/tmp/lt_fuse_gate}; mkdir -p $out
src=/tmp/lt_probe_src; mkdir -p $src
cp lane_tracker_amd/csrc/k_tophat.hip lane_tracker_amd/csrc/k_threshold_walk.hip $src/ || exit 1
patch -s $src/k_tophat.hip tools/probes/k_tophat_vsum.patch && patch -s $src/k_threshold_walk.hip tools/probes/k_threshold_walk_honly.patch || exit 1
make -C lane_tracker_amd/csrc -j16 > /dev/null || exit 1
cd lane_tracker_amd/csrc
F="-O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden -fvisibility-inlines-hidden -Wall -Wno-unused-function -Wno-unused-result --offload-arch=gfx950 -I."
OBJS="lt_api.o lt_memory.o lt_present.o lt_chain.o lt_gather.o lt_tables.o k_frontend.o k_filter.o k_threshold.o k_adaptive_walk.o k_search.o k_overlay.o"
L="/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -Wl,--version-script=exports.map"
/opt/rocm/bin/hipcc $F -DLT_PROBE_VSUM -c $src/k_tophat.hip -o /tmp/kt_vsum.o || exit 1
/opt/rocm/bin/hipcc $F -DLT_PROBE_VSUM -DLT_PROBE_VSUM_RING_ONLY -c $src/k_tophat.hip -o /tmp/kt_ring.o || exit 1
/opt/rocm/bin/hipcc $F -DLT_PROBE_WALK_H_ONLY -c $src/k_threshold_walk.hip -o /tmp/kw_h.o || exit 1
cp ../liblane_tracker_amd.so /tmp/libgate_base.so
$L -o /tmp/libgate_vsum.so $OBJS /tmp/kt_vsum.o k_threshold_walk.o || exit 1
$L -o /tmp/libgate_ring.so $OBJS /tmp/kt_ring.o k_threshold_walk.o || exit 1
$L -o /tmp/libgate_walkh.so $OBJS k_tophat.o /tmp/kw_h.o || exit 1
cd $root
B="$root/bench.py --full --no-cpu-baseline --no-host-fed --no-stream --no-settings --streams 1"
export TMPDIR=/tmp
for pass in 1 2; do
  for v in base vsum ring walkh; do
    d=$out/${v}_$pass
    (cd /tmp && LANE_TRACKER_AMD_LIB=/tmp/libgate_$v.so timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $d -o t -- python3 $B --steps 5 --warmup 2 > $d.log 2>&1)
    rc=$?; [ $rc -ne 0 ] && { echo "$v $pass rc=$rc"; tail -20 $d.log; exit 1; }
    python3 - "$(find $d -name '*kernel_stats.csv' | head -1)" "$v $pass" <<'PY'
import csv, re, sys
for r in csv.DictReader(open(sys.argv[1])):
    n = r["Name"].replace("lt::(anonymous namespace)::", "")
    if re.search(r"k_morph_runs2<[^>]*true, true, true|k_bilateral_walk", n):
        print("%-8s %.4f ms  %s" % (sys.argv[2], float(r["AverageNs"]) / 1e6, re.sub(r"\(.*", "", n.replace("void ", ""))))
PY
    rm -rf $d
  done
done
for v in base vsum; do
  g=1
  for set in "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE" \
             "SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_WAVES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY"; do
    d=$out/pmc${g}_$v
    (cd /tmp && LANE_TRACKER_AMD_LIB=/tmp/libgate_$v.so timeout -k 10 200 rocprofv3 --pmc $set --output-format csv -d $d -o p -- python3 $B --steps 1 --warmup 1 > $d.log 2>&1)
    rc=$?; [ $rc -ne 0 ] && { echo "pmc $v rc=$rc"; tail -20 $d.log; exit 1; }
    echo "== $v, counter group $g"; python3 tools/pmc_kernels.py $d "true, true, true" "walk_hv"
    rm -rf $d; g=$((g + 1))
  done
done
