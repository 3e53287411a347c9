# End-of-round refresh after the counter passes are in profiles/: smoke, the `bench.py --full` line, the rocprofv3 kernel summary
# of the same command (no --pmc).  Usage: bash tools/final_evidence.sh <tag> <output dir>
tag=${1:-r5f}
out=${2:?usage: bash tools/final_evidence.sh <tag> <output dir>}
mkdir -p "$out" && out=$(cd "$out" && pwd) || exit 1
export TMPDIR=/tmp
cd "$(dirname "$0")/.." || exit 1
python -c "import __graft_entry__ as g; g.smoke()" > $out/${tag}_smoke.txt 2>&1; tail -1 $out/${tag}_smoke.txt
python bench.py --full > $out/${tag}_bench.json 2> $out/${tag}_bench.err; tail -c 300 $out/${tag}_bench.json; echo
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $out/${tag}_prof -- python3 bench.py --full --no-cpu-baseline --steps 1 --warmup 1 > $out/${tag}_bench_under_rocprof.json 2> $out/${tag}_prof.err
python tools/shorten_kernel_stats.py $(ls $out/${tag}_prof/*/*kernel_stats.csv | head -1) > $out/${tag}_kernel_stats.csv
head -6 $out/${tag}_kernel_stats.csv | cut -c1-150
rm -rf $out/${tag}_prof
