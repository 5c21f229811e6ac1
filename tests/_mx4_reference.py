"""float64 reference of the mxfp4_e2m1 stored format (docs/format.md) and the
inputs that reach every branch of it, shared by the mxfp4 tests."""

import numpy as np
import torch

from _mx_reference import edge_values

GRID = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], dtype=np.float64)


def mx4_reference(t: torch.Tensor):
    """(payload uint8, decoded float64, E per element) of ``t``'s row-major
    elements, by frexp / ldexp in float64."""
    x = t.detach().cpu().reshape(-1).to(torch.float64).numpy()
    n = x.size
    nb = -(-n // 32)
    x = np.concatenate([x, np.zeros(32 * nb - n)]).reshape(nb, 32)
    finite = np.isfinite(x)
    amax = np.where(finite, np.abs(x), 0.0).max(axis=1)
    E = np.frexp(amax)[1].astype(np.int32) - 3  # floor(log2 amax) - 2
    E = E + (np.ldexp(amax, -E) > 6)
    E = np.maximum(np.where(amax == 0, -127, E), -127).astype(np.int32)
    y = np.minimum(np.ldexp(np.where(finite, np.abs(x), 0.0), -E[:, None]), 6)
    # the grid's step at y: 2^(floor(log2 y) - 1), and 2^-1 below 1
    step = np.ldexp(1.0, np.maximum(np.frexp(y)[1] - 1, 0) - 1)
    q = np.rint(y / step) * step  # rint rounds ties to even
    mag = np.where(finite, np.searchsorted(GRID, q), 7)
    assert np.all(GRID[np.where(finite, mag, 0)] == np.where(finite, q, 0))
    codes = (mag | (np.signbit(x) << 3)).astype(np.uint8)
    X = np.where(finite.all(axis=1), E + 127, 0xFF).astype(np.uint8)
    packed = codes[:, 0::2] | (codes[:, 1::2] << 4)
    payload = torch.from_numpy(np.concatenate([packed.reshape(-1), X]))
    decoded = np.ldexp(np.where(np.signbit(x), -1.0, 1.0) * GRID[mag & 7], E[:, None])
    decoded = np.where((X == 0xFF)[:, None], np.nan, decoded).reshape(-1)[:n]
    return payload, torch.from_numpy(decoded), torch.from_numpy(np.repeat(E, 32)[:n])


def assert_error_bound(t, decoded, E):
    """|decoded - x| <= max(|x| / 4, 2^(E-2)) in blocks of finite elements."""
    x = t.detach().cpu().reshape(-1).to(torch.float64)
    ok = ~torch.isnan(decoded)
    bound = torch.maximum(x.abs() * 2.0**-2, torch.ldexp(torch.ones_like(x), E - 2))
    assert bool(((decoded - x).abs() <= bound)[ok].all())


def edge_values4(n: int, dtype: torch.dtype) -> torch.Tensor:
    """``n`` elements of ``dtype``: five blocks for fp4's own branches, then
    ``edge_values``."""
    g = torch.Generator().manual_seed(n)
    small = torch.rand(32, generator=g) * 5  # below the amax each block names
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    blocks = [
        torch.cat([ties, -ties, torch.tensor([6.0, -0.0]), small[:16]]),  # E = 0
        small.clone(),  # amax exactly 6 * 2^3: no bump
        small * 2.0**-7,  # the next float above 6 * 2^-5: bump
        small.clone(),  # amax 7 * 2^2
        small.clone(),  # -Inf alone makes the block NaN
    ]
    blocks[1][7] = -48.0
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    above = (torch.tensor([6.0 * 2.0**-5], dtype=dtype).view(bits) + 1).view(dtype)
    blocks[2][0] = float(above)
    blocks[3][30] = 28.0
    blocks[4][11] = -float("inf")
    head = torch.cat(blocks).to(dtype)
    return torch.cat([head, edge_values(max(n - head.numel(), 0), dtype)])[:n]
