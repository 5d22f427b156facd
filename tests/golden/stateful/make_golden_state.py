"""Generate tests/golden/stateful/*.npz by running the REFERENCE's own ConvLSTM (build container only): the fixtures of the
stateful path (tests/test_stateful.py).  Same conventions as tests/golden/make_golden.py, whose loader of the reference's
modules and synthetic-weight generator this script reuses.

    python tests/golden/stateful/make_golden_state.py                       # rewrites every fixture
    python tests/golden/stateful/make_golden_state.py convlstm_state.npz    # rewrites the named ones
"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent


def _base():
    """tests/golden/make_golden.py as a module (it loads the reference's modules under private names)."""
    spec = importlib.util.spec_from_file_location("_make_golden", HERE.parent / "make_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def convlstm_state_fixture(name, wseed=33, seed=7):
    """ConvLSTM.forward(x, hidden_state) with a NON-ZERO initial state (reference models/video_autoencoder.py:127-166):
    two layers of different width (32 -> 32 -> 40) on an 8x8 grid, B = 2, T = 3, rolled out in one call and as T = 2 then
    T = 1 with the returned state carried."""
    base = _base()
    stack = base.ref_vae.ConvLSTM(input_dim=32, hidden_dims=[32, 40], kernel_size=3, num_layers=2, return_all_layers=True)
    st = base.synth.synthetic_state({k: tuple(v.shape) for k, v in stack.state_dict().items()}, wseed)
    stack.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()})
    stack.eval()
    rng = np.random.default_rng(seed)
    xs = rng.standard_normal((2, 3, 32, 8, 8), dtype=np.float32)
    state = [(rng.standard_normal((2, hd, 8, 8), dtype=np.float32) * 0.5, rng.standard_normal((2, hd, 8, 8), dtype=np.float32))
             for hd in (32, 40)]
    tstate = [(torch.from_numpy(h), torch.from_numpy(c)) for h, c in state]
    with torch.no_grad():
        outs, finals = stack(torch.from_numpy(xs), tstate)
        outs_a, mid = stack(torch.from_numpy(xs[:, :2]), tstate)
        outs_b, finals_b = stack(torch.from_numpy(xs[:, 2:]), mid)
    arrays = dict(wseed=np.array(wseed), seed=np.array(seed), xs=xs)
    for l in range(2):
        arrays.update({f"h_in{l}": state[l][0], f"c_in{l}": state[l][1], f"seq{l}": outs[l].numpy(),
                       f"h_out{l}": finals[l][0].numpy(), f"c_out{l}": finals[l][1].numpy(),
                       f"h_mid{l}": mid[l][0].numpy(), f"c_mid{l}": mid[l][1].numpy(),
                       f"seq_split{l}": torch.cat([outs_a[l], outs_b[l]], dim=1).numpy(),
                       f"h_out_split{l}": finals_b[l][0].numpy(), f"c_out_split{l}": finals_b[l][1].numpy()})
    path = HERE / name
    np.savez_compressed(path, **arrays)
    print(f"{name}: {path.stat().st_size / 1024:.0f} KiB")


FIXTURES = {
    "convlstm_state.npz": convlstm_state_fixture,
}

if __name__ == "__main__":
    torch.set_num_threads(8)
    for fixture in (sys.argv[1:] or list(FIXTURES)):
        FIXTURES[fixture](fixture)
