"""Inputs of tests/golden/resize_formats/pil_formats.npz: the one-byte (PIL mode L) and four-byte (RGBA) frames of the device
Resize's other pixel formats, regenerated - the fixture stores PIL's outputs only.  Shared by tests/test_resize_formats_plan.py
(CPU), tests/test_hip_resize_formats.py (GPU) and tests/golden/resize_formats/make_golden_resize_formats.py; numpy only.

What the device computes is stated with tests/resize_ref.py::resize_ref, which tests/test_resize_plan.py pins to PIL for RGB:
    l -> 3 channels   resize_ref(g[..., None])           in all three channels     = fromarray(g, 'L').convert('RGB').resize
    l -> 1 channel    resize_ref(g[..., None])                                     = fromarray(g, 'L').resize
    rgba              resize_ref(a[..., :3])                                       = fromarray(a, 'RGBA').convert('RGB').resize
    bgra              the same bytes for the input with B and R exchanged
"""
from __future__ import annotations

import numpy as np

import resize_ref as R

# the cases of resize_ref.CASES the fixture covers: odd sizes, up-scaling, each skipped pass, the copy, the 64-fold cap, a batch
NAMES = ("odd_37x53", "up_128", "horizontal_only", "vertical_only", "copy_64", "cap_down64_up", "240p_64_x6")


def geometry(name: str):
    """(frames, in_h, in_w, out_h, out_w)"""
    return R.CASES[name][2:]


def mono_input(name: str) -> np.ndarray:
    """uint8 [n, in_h, in_w]: hash noise, one byte per pixel."""
    _, seed, n, in_h, in_w, _, _ = R.CASES[name]
    return np.ascontiguousarray(R._synth().frames_u8(seed, 0, n, 1, in_h, in_w)[:, 0])


def rgba_input(name: str) -> np.ndarray:
    """uint8 [n, in_h, in_w, 4]: hash noise in all four bytes (an alpha that entered a sum would show)."""
    _, seed, n, in_h, in_w, _, _ = R.CASES[name]
    return np.ascontiguousarray(R._synth().frames_u8(seed, 0, n, 4, in_h, in_w).transpose(0, 2, 3, 1))


def plane_ref(g: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """uint8 [H, W] -> uint8 [out_h, out_w]: the restatement on one channel."""
    return R.resize_ref(g[..., None], out_h, out_w)[..., 0]


def l_ref(g: np.ndarray, out_h: int, out_w: int, out_channels: int = 3) -> np.ndarray:
    """uint8 [H, W] -> uint8 [out_h, out_w, out_channels]: the resized plane, replicated."""
    return np.ascontiguousarray(np.repeat(plane_ref(g, out_h, out_w)[..., None], out_channels, axis=-1))


def rgba_ref(a: np.ndarray, out_h: int, out_w: int, bgra: bool = False) -> np.ndarray:
    """uint8 [H, W, 4] -> uint8 [out_h, out_w, 3] RGB."""
    rgb = a[..., 2::-1] if bgra else a[..., :3]
    return R.resize_ref(np.ascontiguousarray(rgb), out_h, out_w)


def swap_br(a: np.ndarray) -> np.ndarray:
    """RGBA <-> BGRA (alpha stays the fourth byte)."""
    return np.ascontiguousarray(a[..., [2, 1, 0, 3]])
