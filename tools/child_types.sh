#!/bin/bash
# What the merges of the headline workload merge (coded leaves, internal nodes, cherries) -- no GPU: the checker's sweeps replayed
# on the CPU by tests/probe_child_types.py (tools/ does not import the checker; it shells out) -- and what the merge's site-pattern
# form has to work with: the alignment's distinct columns U, the 64-site steps of a row before (S) and after (U), and whether the
# rule takes the form (phylo_amd/csrc/phylo_site_patterns.h, through the library's debug entries).  From the repo root:
#   tools/child_types.sh [--dataset primate_data] [--K 2048] [--seeds 0 1 2]
set -euo pipefail
REPO=$(cd "$(dirname "$0")/.." && pwd)
python3 "$REPO/tests/probe_child_types.py" "$@"
PYTHONPATH="$REPO${PYTHONPATH:+:$PYTHONPATH}" python3 - "$@" <<'PY'
import argparse
import numpy as np
from phylo_amd import _ffi
from phylo_amd.datasets import load_dataset
p = argparse.ArgumentParser()
p.add_argument('--dataset', default='primate_data')
a, _ = p.parse_known_args()
g = load_dataset(a.dataset)['genome']
N, S, _ = g.shape
coded = bool((((g == 1).sum(axis=2) == 1) & ((g == 0).sum(axis=2) == 3) | ((g == 1).sum(axis=2) == 4)).all())
if not coded:
    print("site patterns: %s has a row that is neither one-hot nor all-ones: no codes, no patterns" % a.dataset)
else:
    codes = np.where(g.sum(axis=2) == 4, 4, g.argmax(axis=2)).astype(np.uint8)
    U = _ffi.debug_site_patterns(codes)["U"]
    ntiles = -(-S // _ffi.load().phylo_site_tile(S))
    print("site patterns: %d distinct columns of %d sites; 64-site steps %d -> %d; form %s by the rule" % (
        U, S, -(-S // 64), -(-U // 64), "taken" if _ffi.debug_site_patterns_rule(S, U, True, ntiles) else "not taken"))
PY
