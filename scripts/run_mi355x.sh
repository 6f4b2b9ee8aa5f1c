#!/bin/bash
# The stages of the reference's run.sh (equilibrate, restart + collect, parse, structural histograms) on the MI355X
# modules of this repository.  Same flags; the cluster flags of the reference (-c -nw -nt -mt ...) are accepted and ignored.
#   scripts/run_mi355x.sh [supercell=5] [pressures=32] [temperatures=32] [cycles=1024] [-ad [-ac CUTOFF]] [-sf [-sq QMAX]]
# Anything after the fourth argument goes to the distr stage: -ad adds the angular distribution (.a.npy / .adf.npy), -ac its
# neighbour shell as a fraction of the smallest box edge (first fcc shell: about 0.85 / supercell); -sf adds the static structure
# factor on the box's reciprocal lattice (.q.npy / .sf.npy / .sfm.npy, and .nrho.npy), -sq its largest index (1..32, default 16).
# REWEIGHT=1 in the environment adds a fifth stage: the multistate reweighting of the grid (.rw*.npy: free energies, H(T), V(T), Cp(T)
# and the temperature of its peak at every pressure); REWEIGHT_ARGS goes to it (e.g. "-sk 128 -ob sof sol" behind a distr stage with -so;
# add "-bs 200" for block-bootstrap error bars on every curve and on the transition temperatures: .rw?s.npy, .rwms.npy, .rwes.npy).
# For several GPUs start the first two stages under  python -m torch.distributed.run --nproc-per-node N -m neuralmelting_amd.remcmc ...
set -euo pipefail
s=${1:-5}; pn=${2:-32}; tn=${3:-32}; sn=${4:-1024}
if [ $# -gt 4 ]; then shift 4; else shift $#; fi
root=$(cd "$(dirname "$0")/.." && pwd)
export PYTHONPATH="$root${PYTHONPATH:+:$PYTHONPATH}"
mkdir -p ./output/remcmc_$s
cd ./output/remcmc_$s
# equilibration run (nothing recorded: cutoff = number of cycles), restart dump at the end
python -m neuralmelting_amd.remcmc -v -n remcmc_init_$s -ss $s -bm -pn $pn -tn $tn -sn $sn -sc $sn -rd $sn
# data collection run, started from that dump
python -m neuralmelting_amd.remcmc -v -r -rn remcmc_init_$s -rs $sn -n remcmc_run_$s -ss $s -bm -pn $pn -tn $tn -sn $sn -rd $sn
# text -> arrays
python -m neuralmelting_amd.parse -v -n remcmc_run_$s
# radial and cartesian pair histograms (and, with -ad, the angular distribution; with -sf, the structure factor)
python -m neuralmelting_amd.distr -v -n remcmc_run_$s -cb 11 "$@"
# optional: free energies and H(T), V(T), Cp(T) between the sampled temperatures (exit status 1 if the iteration did not converge)
if [ "${REWEIGHT:-0}" = 1 ]; then
  python -m neuralmelting_amd.reweight -v -n remcmc_run_$s ${REWEIGHT_ARGS:-}
fi
