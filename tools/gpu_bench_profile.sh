# Runs on the GPU box: full gpu test suite, smoke, bench, and the rocprofv3 kernel stats of the bench command.
# usage: bash tools/gpu_bench_profile.sh [OUTDIR]   (relative to the repository root; default profile_out, git-ignored)
set -e
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=${1:-profile_out}
mkdir -p $O/prof
make -C oracle > /dev/null
python -m pytest tests -m gpu -x -q 2>&1 | tail -5
python -c "import __graft_entry__ as g; g.smoke()"
python bench.py --full --steps 3 --warmup 1 | tee $O/bench.json
rocprofv3 --kernel-trace --stats -d $O/prof -o bench --output-format csv -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extras > $O/prof/bench_prof.log 2>&1
tail -2 $O/prof/bench_prof.log
