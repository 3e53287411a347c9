# Round evidence on one MI355X box: smoke, the `bench.py --full` line, the rocprofv3 kernel summary of the
# same command, and the two PMC passes (FETCH_SIZE / WRITE_SIZE, separate runs, no trace domains besides the kernel trace).
# The counter passes use a 62-frame stack (61 pairs = 3 Farneback batches of 20 / 21 pairs, the batch size of the full
# 144-frame run): rocprofiler's counter collection does not survive ~10^4 dispatches per process on this stack
# (profiles/README.md), a full config-F step has ~10.5 k.  Usage: bash tools/round_evidence.sh <tag> <output dir>
tag=${1:-r6}
out=${2:?usage: bash tools/round_evidence.sh <tag> <output dir>}
mkdir -p "$out" && out=$(cd "$out" && pwd) || exit 1
export TMPDIR=/tmp
cd "$(dirname "$0")/.." || exit 1
python -c "import __graft_entry__ as g; g.smoke()" > $out/${tag}_smoke.txt 2>&1; tail -1 $out/${tag}_smoke.txt
python bench.py --full > $out/${tag}_bench.json 2> $out/${tag}_bench.err; tail -c 400 $out/${tag}_bench.json; echo
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $out/${tag}_prof -- python3 bench.py --full --no-cpu-baseline --steps 1 --warmup 1 > $out/${tag}_bench_under_rocprof.json 2> $out/${tag}_prof.err
python tools/shorten_kernel_stats.py $(ls $out/${tag}_prof/*/*kernel_stats.csv | head -1) > $out/${tag}_kernel_stats.csv
head -8 $out/${tag}_kernel_stats.csv | cut -c1-150
rm -rf $out/${tag}_prof
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 600 rocprofv3 --pmc $c --output-format csv -d $out/${tag}_pmc_$c -- python3 bench.py --frames 62 --n-windows 5 --steps 1 --warmup 0 --no-cpu-baseline --no-raster-subreport > $out/${tag}_pmc_$c.json 2> $out/${tag}_pmc_$c.err || echo "pmc pass $c failed"
done
python tools/pmc_traffic_json.py $out/${tag}_pmc_FETCH_SIZE $out/${tag}_pmc_WRITE_SIZE $out/${tag}_pmc_traffic_bench.json $out/${tag}_pmc_FETCH_SIZE.json | head -8
rm -rf $out/${tag}_pmc_FETCH_SIZE $out/${tag}_pmc_WRITE_SIZE
# VALU issue floor per kernel (round 4): wave-level VALU instructions, waves and busy cycles of the same reduced step
timeout -k 10 600 rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES GRBM_GUI_ACTIVE --output-format csv -d $out/${tag}_pmc_VALU -- python3 bench.py --frames 62 --n-windows 5 --steps 1 --warmup 0 --no-cpu-baseline --no-raster-subreport > $out/${tag}_pmc_VALU.json 2> $out/${tag}_pmc_VALU.err || echo "pmc pass VALU failed"
python tools/pmc_valu_json.py $out/${tag}_pmc_VALU $out/${tag}_pmc_valu_bench.json $out/${tag}_pmc_VALU.json | head -10
rm -rf $out/${tag}_pmc_VALU
