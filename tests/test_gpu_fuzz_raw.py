"""GPU (-m gpu): seeded fuzz of the EVT3 / EVT2 decoder against the sequential restatement (tests/_raw_np.py), bitwise.  Each case
is 3 to 5 chunks of words, decoded whole and in two parts at a random cut with the state carried.  Even seeds draw structured
streams from the word-level generator (tests/_raw_streams.py); odd seeds draw uniformly random words -- every 16- / 32-bit
pattern is legal input and must decode to what the rules say."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _raw_np as R  # noqa: E402
import _raw_streams as G  # noqa: E402
from _raw_streams import same  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import event_utils_amd as E
    from event_utils_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return E


def _case(E, fmt, seed):
    from event_utils_amd import _lib
    C = _lib.EVK_RAW_CHUNK
    rng = np.random.default_rng(1000 * fmt + seed)
    n = int(rng.integers(3 * C, 5 * C + 1))
    if seed % 2:
        words = G.random_words(rng, n, fmt)
    else:
        words = (G.structured_evt3 if fmt == 3 else G.structured_evt2)(rng, n, start_time=bool(rng.integers(0, 4)))
    dec, rdec = (E.decode_evt3, R.decode_evt3) if fmt == 3 else (E.decode_evt2, R.decode_evt2)
    sensor = (720, 1280) if seed % 4 >= 2 else None
    kw = {} if sensor is None else {"sensor_size": sensor, "on_out_of_range": "keep"}
    whole = rdec(words, sensor_size=sensor)
    out, st = dec(words, return_state=True, **kw)
    same(out, st, whole)
    k = int(rng.integers(1, n))
    ra = rdec(words[:k], sensor_size=sensor)
    a, sa = dec(words[:k], return_state=True, **kw)
    same(a, sa, ra)
    b, sb = dec(words[k:], state=sa, return_state=True, **kw)
    same(b, sb, rdec(words[k:], state=ra[5], sensor_size=sensor))
    for c in range(4):
        assert torch.equal(torch.cat((a[c], b[c])), out[c])
    assert tuple(sb) == whole[5] and tuple(u + v for u, v in zip(a.stats, b.stats)) == whole[4]


@pytest.mark.parametrize("seed", range(20))
def test_fuzz_evt3(E, seed):
    _case(E, 3, seed)


@pytest.mark.parametrize("seed", range(20))
def test_fuzz_evt2(E, seed):
    _case(E, 2, seed)
