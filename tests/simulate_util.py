"""Shared by tests/test_simulate.py and tests/test_hip_simulate.py: the tests' inputs for multi_stylegan_amd/simulate.py, an
independent float64 numpy statement of the export's definition, and the round-trip bound of DESIGN 5 ("Simulated datasets")."""
import numpy as np
import torch

GFP, RFP = (150.0, 2200.0), (20.0, 2000.0)
#: one rint contributes at most 0.5 counts; the export's multiply and its add at most half an fp32 ulp at 2^16 each (2^-9); the
#: reader's divide a relative 2^-24.  2^-6 is slack over that sum.
ROUND_TRIP_BOUND = 0.5 + 2.0 ** -6
TIE_WINDOW = 2.0 ** -6                      # fp32 against float64 counts may differ only this close to a tie
RANGE_PRESETS = [(0, 65535), (1000, 1001), (0, 1), (65534, 65535), (150, 4000), (20000, 60000), (0, 300), (4095, 65535)]


def ranges_for(B, T, shift=0):
    """int32 [B, T, 2] count ranges that differ from frame to frame: lo = 0, hi = 65535 and hi = lo + 1 among them."""
    pairs = [RANGE_PRESETS[(k + shift) % len(RANGE_PRESETS)] for k in range(B * T)]
    return torch.tensor(pairs, dtype=torch.int32).reshape(B, T, 2)


def clean_frames(shape, seed=0):
    """fp32 values over [-0.2, 1.2]: no NaN, no infinity."""
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed + sum(shape))) * 1.4 - 0.2


def edge_frames(shape, dtype=torch.float32, seed=0):
    """Values over [-0.2, 1.2] with, at the front of every frame as far as they fit: NaN, 0, 1, the fp32 neighbours just outside
    [0, 1], -0.2 and 1.2 (so x == m and x == M exactly).  Frame j (flat over [B, C, T]) also holds +inf when j % 4 == 1 and -inf
    when j % 4 == 3, and frame 2 is constant but for its NaN."""
    B, C, T, H, W = shape
    x = clean_frames(shape, seed).reshape(B * C * T, H * W)
    front = torch.tensor([float("nan"), 0.0, 1.0, float(np.nextafter(np.float32(0), np.float32(-1))),
                          float(np.nextafter(np.float32(1), np.float32(2))), -0.2, 1.2], dtype=torch.float32)[:H * W]
    x[:, :front.numel()] = front
    for j in range(x.shape[0]):
        if j == 2:
            x[j, 1:] = 0.37
        elif j % 4 == 1 and H * W > 7:
            x[j, 7] = float("inf")
        elif j % 4 == 3 and H * W > 7:
            x[j, 7] = float("-inf")
    return x.reshape(shape).to(dtype)


def reference_values(x, ranges, vflip, gfp=GFP, rfp=RFP, bf_normalise=True):
    """The definition in float64 numpy, written from the issue's text and not from the package: x [B, C, T, H, W] (any float
    tensor, widened exactly), ranges int [B, T, 2] -> float64 [B, C, T, H, W] values BEFORE rint (NaN where the count is 0 by
    the NaN rule)."""
    x = x.to(torch.float64).numpy()
    ranges = np.asarray(ranges, dtype=np.float64)
    B, C, T, H, W = x.shape
    v = np.empty_like(x)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for b in range(B):
            for t in range(T):
                frame, (lo, hi) = x[b, 0, t], ranges[b, t]
                if bf_normalise:
                    finite = frame[~np.isnan(frame)]
                    m, M = (finite.min(), finite.max()) if finite.size else (np.inf, -np.inf)
                    n = np.where(np.isnan(frame), np.nan, 0.0) if M == m else (frame - m) / (M - m)
                else:
                    n = np.clip(frame, 0.0, 1.0)
                v[b, 0, t] = n * (hi - lo) + lo
        for c, (low, div) in zip(range(1, C), (gfp, rfp)):
            v[:, c] = np.clip(x[:, c], 0.0, 1.0) * div + low
    return v[:, :, :, ::-1] if vflip else v


def counts_of(values):
    """rint (numpy's: ties to even), NaN -> 0, clamped to [0, 65535]."""
    return np.clip(np.nan_to_num(np.rint(values), nan=0.0, posinf=65535.0, neginf=0.0), 0, 65535).astype(np.int64)


def assert_close_to_reference(counts, values):
    """fp32 counts against the float64 values: at most one count apart, only where the float64 value lies within TIE_WINDOW of a
    tie, and on at most 1 % of the pixels."""
    got, want = np.asarray(counts).astype(np.int64), counts_of(values)
    differ = got != want
    assert np.abs(got - want).max() <= 1, np.abs(got - want).max()
    if differ.any():
        at = values[differ]
        assert np.all(np.abs(np.abs(at - np.floor(at)) - 0.5) <= TIE_WINDOW), at[:8]
    assert differ.mean() <= 0.01, differ.mean()
    return int(differ.sum())


def definition_n(x):
    """The definition's n of clean bright-field frames [B, T, H, W] in fp32: (x - m) / (M - m)."""
    flat = x.flatten(start_dim=2)
    m, M = flat.amin(dim=2).view(*x.shape[:2], 1, 1), flat.amax(dim=2).view(*x.shape[:2], 1, 1)
    return (x - m) / (M - m)


def assert_round_trip(x, ranges, counts, back, gfp=GFP, rfp=RFP):
    """``back`` = the reader's normalisation of ``counts`` = the export of clean fp32 frames ``x``: within ROUND_TRIP_BOUND counts
    of the definition's n (bright field; its counts span [lo, hi] exactly) and of clamp(x, 0, 1) (GFP / RFP).  -> the two worst
    cases in counts."""
    x, back = x.to(torch.float32).cpu(), back.to(torch.float32).cpu()
    counts = counts.cpu().numpy()
    B, C, T, H, W = x.shape
    span = (ranges[..., 1] - ranges[..., 0]).to(torch.float64).view(B, T, 1, 1)
    worst_bf = ((back[:, 0].double() - definition_n(x[:, 0]).double()).abs() * span).max().item()
    assert worst_bf <= ROUND_TRIP_BOUND, worst_bf
    assert np.array_equal(counts[:, 0].reshape(B, T, -1).min(axis=2), ranges[..., 0].numpy())
    assert np.array_equal(counts[:, 0].reshape(B, T, -1).max(axis=2), ranges[..., 1].numpy())
    worst_fl = 0.0
    for c, (low, div) in zip(range(1, C), (gfp, rfp)):
        worst_fl = max(worst_fl, ((back[:, c].double() - x[:, c].clamp(0.0, 1.0).double()).abs() * div).max().item())
    assert worst_fl <= ROUND_TRIP_BOUND, worst_fl
    return worst_bf, worst_fl
