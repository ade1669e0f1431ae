"""Balanced epochs without a GPU (cova_amd/train.py, balanced_samples): the draw against a plain-Python restatement, its
determinism, the in-order walk with wrap of each half, the refusals, the command line, and the NULL checks of
covahip_train_data_label_mass."""

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import train as T

M = (1 << 64) - 1
INVALID_ARG = 1


def _sm(z):
    z = (z + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def _restated(samples, mass, threshold, mass_first, data_seed, epoch, model):
    """The issue's definition, one draw at a time: indices into `samples`."""
    busy = [int(mass[int(s["label"]) - mass_first]) >= threshold for s in samples]
    b = [i for i, x in enumerate(busy) if x]
    q = [i for i, x in enumerate(busy) if not x]
    key = _sm((data_seed & M) ^ _sm((epoch << 20 | model << 4 | 5) & M))
    out, nb, nq = [], 0, 0
    for j in range(len(samples)):
        if _sm((key + j) & M) >> 63:
            out.append(b[nb % len(b)])
            nb += 1
        else:
            out.append(q[nq % len(q)])
            nq += 1
    return out, nb


def _samples(n, first=0, seed=0, reverse=True):
    """n distinct samples with newest frames first + 3 .. first + n + 2, in a shuffled order; with `reverse` three in ten are
    listed oldest first (two samples may then share a labelling frame)."""
    rng = np.random.default_rng(seed)
    k = first + 3 + rng.permutation(n)
    s = np.zeros(n, T.SAMPLE)
    s["frame"] = k[:, None] - np.arange(4)[None, :]
    s["label"] = k
    s["flags"] = rng.integers(0, 4, n)
    rev = (rng.random(n) < 0.3) & reverse
    s["frame"][rev] = s["frame"][rev][:, ::-1]
    s["label"][rev] = s["frame"][rev][:, 0]                               # the oldest frame labels a reversed window
    return s


@pytest.mark.parametrize("data_seed,epoch,model", [(0, 0, 0), (12345, 3, 2), (M, 40, 255)])
def test_balanced_samples_is_the_stated_function(data_seed, epoch, model):
    n, first = 400, 11
    s = _samples(n, first, 1)
    mass = np.random.default_rng(2).integers(0, 200, n + 3).astype(np.uint32)     # frames first .. first + n + 2
    got = T.balanced_samples(s, mass, 100, mass_first=first, data_seed=data_seed, epoch=epoch, model=model)
    want, nb = _restated(s, mass, 100, first, data_seed, epoch, model)
    assert got.dtype == T.SAMPLE and got.shape == (n,) and got.flags["C_CONTIGUOUS"]
    assert got.tobytes() == s[want].tobytes()
    again = T.balanced_samples(s, mass, 100, mass_first=first, data_seed=data_seed, epoch=epoch, model=model)
    assert again.tobytes() == got.tobytes()
    # the restatement alone: a fair coin's share of 400 draws, within 4 sigma
    assert 0.4 <= nb / n <= 0.6, nb
    busy = mass[got["label"] - first] >= 100
    assert int(busy.sum()) == nb


def test_epochs_models_and_seeds_draw_differently():
    s = _samples(200, 0, 3)
    mass = np.random.default_rng(4).integers(0, 200, 203).astype(np.uint32)
    base = T.balanced_samples(s, mass, 100, data_seed=1, epoch=0, model=0).tobytes()
    assert T.balanced_samples(s, mass, 100, data_seed=1, epoch=1, model=0).tobytes() != base
    assert T.balanced_samples(s, mass, 100, data_seed=1, epoch=0, model=1).tobytes() != base
    assert T.balanced_samples(s, mass, 100, data_seed=2, epoch=0, model=0).tobytes() != base
    for kw in (dict(model=1 << 16), dict(model=-1), dict(epoch=1 << 44), dict(epoch=-1)):     # the key's fields would overlap
        with pytest.raises(ValueError):
            T.balanced_samples(s, mass, 100, **kw)


def test_each_half_is_walked_in_order_and_wraps():
    n = 200
    s = _samples(n, 0, 5, reverse=False)                                  # every sample has a labelling frame of its own
    mass = np.zeros(n + 3, np.uint32)
    three = [int(s["label"][i]) for i in (17, 90, 150)]                   # three busy samples, in this order
    mass[three] = 7
    out = T.balanced_samples(s, mass, 7, data_seed=9, epoch=2, model=1)
    assert len(out) == n
    is_busy = np.isin(out["label"], three)
    assert 80 <= int(is_busy.sum()) <= 120                                # 4 sigma of 200 fair draws: the three wrap ~30 times
    assert out["label"][is_busy].tolist() == [three[i % 3] for i in range(int(is_busy.sum()))]
    quiet = s[~np.isin(s["label"], three)]
    nq = int((~is_busy).sum())
    assert out[~is_busy].tobytes() == quiet[np.arange(nq) % len(quiet)].tobytes()
    # the other way round: three quiet samples among busy ones
    out = T.balanced_samples(s, 7 - mass, 7, data_seed=9, epoch=2, model=1)
    is_quiet = np.isin(out["label"], three)
    assert out["label"][is_quiet].tolist() == [three[i % 3] for i in range(int(is_quiet.sum()))] and int(is_quiet.sum()) > 3


def test_a_drawn_sample_keeps_its_mirrors_and_direction():
    table = T.windows([(0, 40)], "overlap")
    e = T.epoch_samples(table, (1,), 3, 1, 0, True, "xy", True)
    mass = (np.arange(40) % 5 == 0).astype(np.uint32) * 50
    out = T.balanced_samples(e, mass, 50, data_seed=3, epoch=1, model=0)
    rows = {r.tobytes() for r in e}
    assert all(r.tobytes() in rows for r in out) and len({r.tobytes() for r in out}) < len(out)    # whole records, some twice


def test_an_empty_half_is_refused_with_both_counts():
    s = _samples(20, 0, 6)
    for mass, msg in ((np.full(23, 5, np.uint32), "20 busy and 0 quiet"), (np.zeros(23, np.uint32), "0 busy and 20 quiet")):
        with pytest.raises(ValueError) as e:
            T.balanced_samples(s, mass, 5)
        assert msg in str(e.value) and "threshold 5" in str(e.value)


def test_mass_first_is_honoured():
    n, first = 50, 1000
    s = _samples(n, first, 7)
    mass = np.random.default_rng(8).integers(0, 10, n + 3).astype(np.uint32)
    got = T.balanced_samples(s, mass, 5, mass_first=first, data_seed=4)
    shifted = s.copy()
    shifted["label"] -= first
    shifted["frame"] -= first
    want = T.balanced_samples(shifted, mass, 5, data_seed=4)
    assert (got["label"] - first).tolist() == want["label"].tolist() and got["flags"].tolist() == want["flags"].tolist()
    for bad_first in (first + n + 3, first - 2 * n):                            # the masses do not cover the labelling frames
        with pytest.raises(ValueError):
            T.balanced_samples(s, mass, 5, mass_first=bad_first)
    with pytest.raises(ValueError):
        T.balanced_samples(s.astype([("frame", "<i4", (4,)), ("label", "<i8"), ("flags", "<u4")]), mass, 5, mass_first=first)


def test_command_line():
    base = ["a.tfrecord", "-o", "o.cvhw"]
    assert T.parse_args(base).resident is False and T.parse_args(base).balance is None
    a = T.parse_args(base + ["--balance", "100"])
    assert a.resident is True and a.balance == 100 and a.windows is None
    for bad in (["--eval-only", "w.cvhw", "a.tfrecord", "--balance", "100"], base + ["--balance", "0"], base + ["--balance", "x"]):
        with pytest.raises(SystemExit) as e:
            T.parse_args(bad)
        assert e.value.code == 2


def test_null_arguments_do_not_need_a_gpu():
    lib = L.lib()
    mass = np.full(4, 0xAAAAAAAA, np.uint32)
    assert lib.covahip_train_data_label_mass(None, 0, 4, None, mass.ctypes.data, L.MEM_HOST) == INVALID_ARG
    assert lib.covahip_train_data_label_mass(None, 0, 4, None, None, L.MEM_HOST) == INVALID_ARG
    assert (mass == 0xAAAAAAAA).all()
