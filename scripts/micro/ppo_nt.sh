# rocprofv3 kernel stats of 2 PPO updates (bench.py) with the product library
# and with DR_PPO_NT=1 (nontemporal activation / grad_z stores);
# logs and traces go to $OUT (default: out/ in the repository)
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
cd /tmp && export TMPDIR=/tmp && cd "$ROOT"
OUT=${OUT:-out}
mkdir -p $OUT
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/pnt0 -o run -- python3 bench.py --full --steps 10 --warmup 5 --no-cpu-baseline --ppo-updates 2 > $OUT/pnt0.log 2>&1 &&
DRONERL_LIB=$ROOT/scripts/micro/build/lib_ppont.so timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/pnt1 -o run -- python3 bench.py --full --steps 10 --warmup 5 --no-cpu-baseline --ppo-updates 2 > $OUT/pnt1.log 2>&1 &&
grep -h '"ppo"' $OUT/pnt0.log $OUT/pnt1.log | python3 -c "import sys,json; [print(json.loads(l)['ppo']['updates_per_s']) for l in sys.stdin]"
