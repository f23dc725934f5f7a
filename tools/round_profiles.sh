# the round's evidence in one GPU call: counter passes (fabric bytes per step, per precision), kernel traces of the four workloads,
# and the full bench line.  usage (on an MI355X): MDM_COMMIT=<short hash> bash tools/round_profiles.sh <tag, e.g. r04> [<bench log>]
TAG=${1:-r04}
LOG=${2:-${TAG}_bench_full.log}
bash tools/pmc_step.sh 1 gpurun_out/${TAG}_pmc_traffic_p1.json > gpurun_out/${TAG}_pmc_p1.log 2>&1 &&
bash tools/pmc_step.sh 3 gpurun_out/${TAG}_pmc_traffic_p3.json > gpurun_out/${TAG}_pmc_p3.log 2>&1 &&
bash tools/profile_step.sh ${TAG}_bf16 > /dev/null 2>&1 &&
bash tools/profile_step.sh ${TAG}_parity --precision 3 > /dev/null 2>&1 &&
bash tools/profile_step.sh ${TAG}_big --config big > /dev/null 2>&1 &&
bash tools/profile_step.sh ${TAG}_big16 --config big16 --batch 8 --precision 2 > /dev/null 2>&1 &&
( time python bench.py --full ) > "$LOG" 2>&1
tail -3 "$LOG" | cut -c1-400
