#!/bin/bash
# What the merges of the headline workload merge (coded leaves, internal nodes, cherries) -- no GPU: the checker's sweeps replayed
# on the CPU by tests/probe_child_types.py (tools/ does not import the checker; it shells out).  From the repo root:
#   tools/child_types.sh [--dataset primate_data] [--K 2048] [--seeds 0 1 2]
set -euo pipefail
REPO=$(cd "$(dirname "$0")/.." && pwd)
exec python3 "$REPO/tests/probe_child_types.py" "$@"
