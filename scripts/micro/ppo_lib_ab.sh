# rocprofv3 kernel stats of 2 PPO updates (bench.py) with the product library
# and with an A/B variant library (arg 1: path under scripts/micro/build);
# logs and traces go to $OUT (default: out/ in the repository)
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
cd /tmp && export TMPDIR=/tmp && cd "$ROOT"
OUT=${OUT:-out}
mkdir -p $OUT
V=$1
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/ab0 -o run -- python3 bench.py --full --steps 10 --warmup 5 --no-cpu-baseline --ppo-updates 2 > $OUT/ab0.log 2>&1 &&
DRONERL_LIB=$ROOT/scripts/micro/build/$V timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/ab1 -o run -- python3 bench.py --full --steps 10 --warmup 5 --no-cpu-baseline --ppo-updates 2 > $OUT/ab1.log 2>&1 &&
grep -h '"ppo"' $OUT/ab0.log $OUT/ab1.log | python3 -c "import sys,json; [print(json.loads(l)['ppo']['updates_per_s']) for l in sys.stdin]"
