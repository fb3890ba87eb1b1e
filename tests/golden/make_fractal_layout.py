"""Writes tests/golden/fractal_easy_layout.json: parameter names / shapes and the fractal config of
the reference's committed checkpoint fractal_experiments/frala_easy_final/final_fractal_agent.pt
(read with torch.load(weights_only=True): no code from the file runs), plus per-tensor sums of the
world-model weights; and the world-model weights themselves as tests/golden/fractal_easy_weights
(.partN.npz, make_golden.save), which tests/test_fractal.py loads strictly.  Run where the reference
tree is at hand, XTRL_REFERENCE naming its root:
    XTRL_REFERENCE=<reference tree> python tests/golden/make_fractal_layout.py
"""
import json
import os
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
from make_golden import save   # noqa: E402

SRC = Path(os.environ['XTRL_REFERENCE']) / 'fractal_experiments' / 'frala_easy_final' / 'final_fractal_agent.pt'
OUT = HERE / 'fractal_easy_layout.json'

ck = torch.load(SRC, weights_only=True, map_location='cpu')
wm = ck['world_model']
layout = {k: list(v.shape) for k, v in wm.items()}
sums = {k: float(v.double().sum()) for k, v in wm.items()}
json.dump(dict(fractal_config=ck['fractal_config'], agent_config={k: v for k, v in ck['agent_config'].items()},
               layout=layout, sums=sums), OUT.open('w'), indent=1, default=list)
print(OUT, len(layout), 'tensors')
save('fractal_easy_weights', **wm)
