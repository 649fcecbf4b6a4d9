"""Writes slowtv_monodepth_amd/cmaps.json (text: a float's repr round-trips float64 exactly): the 256-entry RGB tables of matplotlib's 'turbo', 'magma' and 'viridis' (float64, alpha dropped) and the
matplotlib version they were read from.  Data taken from matplotlib; tests/test_viz_host.py compares the file with the installed matplotlib's tables.
Usage: python scripts/dev/make_cmaps.py"""
import json
from pathlib import Path

import matplotlib
import numpy as np
from matplotlib import pyplot as plt

NAMES = ('turbo', 'magma', 'viridis')

if __name__ == '__main__':
    tables = {}
    for name in NAMES:
        cmap = plt.get_cmap(name)
        table = np.asarray(cmap(np.arange(cmap.N)), dtype=np.float64)[:, :3]                   # integer input indexes the table directly
        assert table.shape == (256, 3)
        tables[name] = table.tolist()
    out = Path(__file__).resolve().parents[2]/'slowtv_monodepth_amd'/'cmaps.json'
    doc = {'generator': 'scripts/dev/make_cmaps.py', 'matplotlib_version': matplotlib.__version__, **tables}
    out.write_text(json.dumps(doc, separators=(',', ':')).replace('],[', '],\n[') + '\n')
    print(f'wrote {out} ({out.stat().st_size} bytes) from matplotlib {matplotlib.__version__}')
