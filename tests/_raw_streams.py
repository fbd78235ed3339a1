"""Word-level generators of EVT3 / EVT2 test streams (no events behind them: the words themselves are drawn), shared by the raw
decoder's GPU tests, and their bitwise comparison.  They use neither the package's encoder nor the restatement."""
import numpy as np

RESERVED3 = (0x1, 0x7, 0x9, 0xB, 0xC, 0xD, 0xE, 0xF)
RESERVED2 = (0x2, 0x3, 0x4, 0x5, 0x6, 0x7, 0x9, 0xB, 0xC, 0xD, 0xE, 0xF)


def structured_evt3(rng, n, start_time=True):
    """n words: a random mix of the types with realistic run lengths -- runs of ADDR_X, VECT_BASE_X with runs of VECT_12 and a
    closing VECT_8, masks from empty to full, TIME_HIGH mostly stepping by one with occasional loops and backward steps, TIME_LOW,
    ADDR_Y, triggers, reserved types"""
    out = []
    th = int(rng.integers(0, 4096))
    if start_time:
        out.append(0x8000 | th)
    while len(out) < n:
        r = rng.random()
        if r < 0.10:
            s = rng.random()
            if s < 0.70:
                th = (th + 1) & 0xFFF                          # (4095 -> 0 is a loop)
            elif s < 0.80:
                th = int(rng.integers(4086, 4096))             # up to the top: the next small value loops
            elif s < 0.90:
                th = max(0, th - int(rng.integers(1, 30)))     # a small step back
            else:
                th = int(rng.integers(0, 4096))
            out.append(0x8000 | th)
        elif r < 0.22:
            out.append(0x6000 | int(rng.integers(0, 4096)))
        elif r < 0.32:
            out.append(0x0000 | int(rng.integers(0, 4096)))    # (bit 11 set at times: ignored)
        elif r < 0.62:
            k = int(rng.integers(1, 24))
            out.extend((0x2000 | rng.integers(0, 4096, k)).tolist())
        elif r < 0.86:
            if rng.random() < 0.85:
                out.append(0x3000 | int(rng.integers(0, 4096)))
            for _ in range(int(rng.integers(1, 8))):
                m = rng.random()
                out.append(0x4000 | (0 if m < 0.1 else 0xFFF if m < 0.25 else int(rng.integers(0, 4096))))
            if rng.random() < 0.5:
                out.append(0x5000 | int(rng.integers(0, 4096)))  # (bits 8-11 set at times: ignored)
        elif r < 0.91:
            out.append(0xA000 | int(rng.integers(0, 4096)))
        else:
            out.append((int(rng.choice(RESERVED3)) << 12) | int(rng.integers(0, 4096)))
    return np.array(out[:n], dtype=np.uint16)


def structured_evt2(rng, n, start_time=True):
    out = []
    th = int(rng.integers(0, 1 << 28))
    if start_time:
        out.append((0x8 << 28) | th)
    while len(out) < n:
        r = rng.random()
        if r < 0.12:
            s = rng.random()
            th = (th + 1) & 0x0FFFFFFF if s < 0.8 else (max(0, th - 3) if s < 0.9 else int(rng.integers(0, 1 << 28)))
            out.append((0x8 << 28) | th)
        elif r < 0.88:
            k = int(rng.integers(1, 40))
            out.extend(((rng.integers(0, 2, k) << 28) | rng.integers(0, 1 << 28, k)).tolist())
        elif r < 0.93:
            out.append((0xA << 28) | int(rng.integers(0, 1 << 28)))
        else:
            out.append((int(rng.choice(RESERVED2)) << 28) | int(rng.integers(0, 1 << 28)))
    return np.array(out[:n], dtype=np.uint32)


def random_words(rng, n, fmt):
    """uniformly random words: every bit pattern is legal input"""
    if fmt == 3:
        return rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16)
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def same(out, state, ref):
    """device result (RawEvents, RawState) == restatement result, bit for bit"""
    for k, dt in enumerate(("torch.int16", "torch.int16", "torch.int64", "torch.uint8")):
        assert str(out[k].dtype) == dt and out[k].is_cuda
        got = out[k].cpu().numpy()
        assert got.shape == ref[k].shape, (k, got.shape, ref[k].shape)
        bad = np.flatnonzero(got != ref[k])
        assert bad.size == 0, (k, bad[:5], got[bad[:5]], ref[k][bad[:5]])
    assert tuple(out.stats) == ref[4], (tuple(out.stats), ref[4])
    assert all(type(v) is int for v in out.stats)
    if state is not None:
        assert tuple(state) == ref[5], (tuple(state), ref[5])
