"""float64 reference of the mxfp8_e4m3 stored format (docs/format.md) and
the inputs that reach every branch of it, shared by the mx tests."""

import numpy as np
import torch


def mx_reference(t: torch.Tensor):
    """(payload uint8, decoded float64, E per element) of ``t``'s row-major
    elements, by frexp / ldexp in float64."""
    x = t.detach().cpu().reshape(-1).to(torch.float64).numpy()
    n = x.size
    nb = -(-n // 32)
    x = np.concatenate([x, np.zeros(32 * nb - n)]).reshape(nb, 32)
    finite = np.isfinite(x)
    amax = np.where(finite, np.abs(x), 0.0).max(axis=1)
    E = np.frexp(amax)[1].astype(np.int32) - 9  # floor(log2 amax) - 8
    E = E + (np.ldexp(amax, -E) > 448)
    E = np.maximum(np.where(amax == 0, -127, E), -127).astype(np.int32)
    y = np.clip(np.ldexp(np.where(finite, x, 0.0), -E[:, None]), -448, 448)
    codes = torch.from_numpy(y).float().to(torch.float8_e4m3fn).view(torch.uint8)
    codes = np.where(finite, codes.numpy(), 0x7F | (np.signbit(x) << 7))
    codes = torch.from_numpy(codes.astype(np.uint8))
    payload = torch.cat([codes.reshape(-1), torch.from_numpy((E + 127).astype(np.uint8))])
    values = codes.view(torch.float8_e4m3fn).float().double().numpy()
    decoded = np.ldexp(values, E[:, None]).reshape(-1)[:n]
    return payload, torch.from_numpy(decoded), torch.from_numpy(np.repeat(E, 32)[:n])


def decoded_as(decoded, dtype):
    """The reference's decoded values as a ``dtype`` target receives them."""
    return decoded.to(torch.float32).to(dtype)


def assert_error_bound(t, decoded, E):
    x = t.detach().cpu().reshape(-1).to(torch.float64)
    ok = torch.isfinite(x)
    bound = torch.maximum(x.abs() * 2.0**-4, torch.ldexp(torch.ones_like(x), E - 10))
    assert bool(((decoded - x).abs() <= bound)[ok].all())


def edge_values(n: int, dtype: torch.dtype) -> torch.Tensor:
    """``n`` elements of ``dtype``: seven blocks of 32 that reach every branch
    of the format, then wide-spread random values."""
    g = torch.Generator().manual_seed(n)
    small = torch.rand(32, generator=g) * 100  # below the amax each block names
    blocks = [
        torch.zeros(32),
        small.clone(),  # finite values beside NaN and both infinities
        torch.full((32,), 2.0**-140) * torch.arange(1, 33),  # f32 subnormals
        small.clone(),  # amax exactly 448 * 2^3: no bump
        small * 2.0**-9,  # the next float above 448 * 2^-5: bump
        torch.tensor([17.0, 19.0, 18.0, 22.0, 26.0, 2.0**-10, 3 * 2.0**-10, 2.0**-11] * 4),
        small * 1e30,  # |x| near 3e38
    ]
    blocks[1][[3, 9, 20]] = torch.tensor([float("nan"), float("inf"), -float("inf")])
    blocks[1][4] = -0.0
    blocks[3][7] = -448.0 * 8
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    above = (torch.tensor([448.0 * 2.0**-5], dtype=dtype).view(bits) + 1).view(dtype)
    blocks[4][0] = float(above)
    blocks[5][31] = 256.0  # E = 0: 17 and 19 are ties at step 2
    blocks[6][[1, 2]] = torch.tensor([3e38, -3e38])
    head = torch.cat(blocks)
    rest = max(n - head.numel(), 0)
    spread = torch.randn(rest, generator=g) * torch.exp2(
        torch.randint(-40, 40, (rest,), generator=g).float()
    )
    return torch.cat([head, spread])[:n].to(dtype)
