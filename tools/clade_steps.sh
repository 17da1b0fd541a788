#!/bin/bash
# The phase-1 steps the clade tables of the merge's site-pattern form leave on a workload (phylo_amd/csrc/phylo_site_patterns.h) -- no
# GPU: the checker's sweeps replayed on the CPU by tests/probe_clade_steps.py (tools/ does not import the checker; it shells out): the
# share of merges that are not leaf x leaf, the histogram of ceil(U_Z / 64) over them and its mean by rank event.  From the repo root:
#   tools/clade_steps.sh [--dataset primate_data] [--K 2048] [--seeds 0 1 2]
set -euo pipefail
REPO=$(cd "$(dirname "$0")/.." && pwd)
python3 "$REPO/tests/probe_clade_steps.py" "$@"
