"""Held-out evaluation and exact resume of BlobNet training, the parts that need no GPU: the C entries refuse bad arguments
before any device work, the tail split, the state blob's header as pure Python reads it, and the command line's argument rules."""
import ctypes as C
import struct

import numpy as np
import pytest

from cova_amd import _lib as L
from cova_amd import train as T
from cova_amd import weights as W


def test_new_entries_refuse_bad_arguments_without_a_gpu():
    lib = L.lib()
    res = L.TrainEvalResult()
    buf = np.zeros(64, np.uint8)
    cnt = np.ones(1, np.int32)
    n = C.c_size_t(123)
    tag = C.c_uint64()
    p = buf.ctypes.data
    # no trainer
    assert lib.covahip_train_eval(None, p, p, 1, None, None, C.byref(res), L.MEM_HOST) == 1
    assert lib.covahip_train_eval_set(None, p, p, cnt.ctypes.data, None, None, C.byref(res), L.MEM_HOST) == 1
    assert lib.covahip_train_state_size(None, C.byref(n)) == 1
    assert lib.covahip_train_save_state(None, 0, p, 64, C.byref(n)) == 1
    assert lib.covahip_train_load_state(None, p, 64, C.byref(tag)) == 1
    assert n.value == 123 and tag.value == 0
    assert C.sizeof(L.TrainEvalResult) == 40


def _data(n, h=2, w=3):
    stacks = np.arange(n * 4 * h * w * 4, dtype=np.uint32).reshape(n, 4 * h, w, 4).astype(np.uint8)
    labels = (np.arange(n * h * w).reshape(n, h, w) % 2).astype(np.uint8)
    stacks[:, 0, 0, 0] = np.arange(n)          # the sample's index, to check the order
    return stacks, labels


@pytest.mark.parametrize("n,frac,n_val", [(10, 0.2, 2), (10, 0.25, 3), (16, 0.25, 4), (10, 0.1, 1), (10, 0.3, 3), (7, 0.5, 4), (3, 0.01, 1),
                                          (10, 0.9, 9)])
def test_split_tail_sizes_and_order(n, frac, n_val):
    stacks, labels = _data(n)
    (tx, ty), (vx, vy) = T.split_tail(stacks, labels, frac)
    assert (tx.shape[0], vx.shape[0]) == (n - n_val, n_val) and ty.shape[0] == n - n_val and vy.shape[0] == n_val
    assert tx[:, 0, 0, 0].tolist() == list(range(n - n_val))              # the head trains, in order
    assert vx[:, 0, 0, 0].tolist() == list(range(n - n_val, n))           # the tail validates, in order
    assert (np.concatenate([ty, vy]) == labels).all()


@pytest.mark.parametrize("n,frac", [(10, 0.0), (10, 1.0), (10, 0.95), (1, 0.5), (10, -0.1), (4, 1.5)])
def test_split_tail_refuses_an_empty_part(n, frac):
    with pytest.raises(ValueError):
        T.split_tail(*_data(n), frac)


def _blob(n_models=2, n_params=5, version=1, magic=T.STATE_MAGIC, tag=7):
    """A state blob built by hand from the layout in include/covahip.h (n_params is the header's to choose here)."""
    out = struct.pack("<IIIIii", magic, version, n_models, n_params, 45, 80)
    out += struct.pack("<8f", 1e-3, 0.9, 0.999, 1e-7, 0.99, 1e-3, 0.2, 100.0)
    out += struct.pack("<Q", tag)
    assert len(out) == 64
    for k in range(n_models):
        out += struct.pack("<QQ", 10 + k, 1000 + k)
        out += np.arange(3 * n_params, dtype=np.float32).tobytes()
    return out + struct.pack("<I", T.crc32c(out))


def test_read_state_header_on_a_hand_built_blob():
    hdr = T.read_state_header(_blob())
    assert (hdr["version"], hdr["n_models"], hdr["n_params"], hdr["h_mb"], hdr["w_mb"], hdr["user_tag"]) == (1, 2, 5, 45, 80, 7)
    assert hdr["steps"] == [10, 11] and hdr["seeds"] == [1000, 1001]
    assert hdr["lr"] == np.float32(1e-3) and hdr["beta2"] == np.float32(0.999) and hdr["dropout"] == np.float32(0.2)
    assert hdr["smooth"] == 100.0 and hdr["bn_momentum"] == np.float32(0.99)
    # the checksum is the TFRecord one, unmasked: CRC-32C of "123456789" is the catalogue's check value
    assert T.crc32c(b"123456789") == 0xE3069283
    # a real trainer's blob has this size
    full = 64 + 3 * (16 + 3 * 4 * W.N_PARAMS) + 4
    assert len(_blob(3, W.N_PARAMS)) == full


def test_read_state_header_names_what_is_wrong():
    good = _blob()
    flipped = bytearray(good)
    flipped[100] ^= 0x10
    with pytest.raises(ValueError, match="CRC mismatch"):
        T.read_state_header(bytes(flipped))
    with pytest.raises(ValueError, match="truncated"):
        T.read_state_header(good[:-9])
    with pytest.raises(ValueError, match="truncated"):
        T.read_state_header(good[:40])
    with pytest.raises(ValueError, match="size mismatch"):
        T.read_state_header(good + b"\0")
    with pytest.raises(ValueError, match="unsupported version 2"):
        T.read_state_header(_blob(version=2))
    with pytest.raises(ValueError, match="bad magic"):
        T.read_state_header(_blob(magic=0x57485643))       # a weight file's magic


def _cli_error(argv, capsys, text):
    with pytest.raises(SystemExit) as e:
        T.parse_args(argv)
    assert e.value.code == 2
    assert text in capsys.readouterr().err


def test_cli_argument_rules(capsys):
    a = T.parse_args(["a.tfrecord", "-o", "out.cvhw"])
    assert (a.val, a.val_frac, a.keep, a.checkpoint, a.resume, a.eval_only) == (None, None, "last", None, None, None)
    a = T.parse_args(["a.tfrecord", "-o", "out.cvhw", "--val-frac", "0.2", "--keep", "best", "--checkpoint", "c.cvhs", "--resume", "c.cvhs"])
    assert (a.val_frac, a.keep, a.checkpoint, a.resume) == (0.2, "best", "c.cvhs", "c.cvhs")
    a = T.parse_args(["--set", "-o", "dir", "a.tfrecord", "b.tfrecord", "--val", "va.tfrecord", "vb1.tfrecord,vb2.tfrecord"])
    assert a.val == ["va.tfrecord", "vb1.tfrecord,vb2.tfrecord"] and a.records == ["a.tfrecord", "b.tfrecord"]
    a = T.parse_args(["--eval-only", "w.cvhw", "today.tfrecord"])
    assert a.eval_only == "w.cvhw" and a.records == ["today.tfrecord"] and a.output is None
    _cli_error(["a.tfrecord", "-o", "o.cvhw", "--keep", "best"], capsys, "--keep best needs validation data")
    _cli_error(["--set", "-o", "dir", "a.tfrecord", "b.tfrecord", "--val", "va.tfrecord"], capsys, "--val names 1 models, the set has 2")
    _cli_error(["--eval-only", "w.cvhw", "a.tfrecord", "--resume", "c.cvhs"], capsys, "--eval-only trains nothing")
    _cli_error(["a.tfrecord", "-o", "o.cvhw", "--val", "v.tfrecord", "--val-frac", "0.2"], capsys, "exclude each other")
    _cli_error(["a.tfrecord", "-o", "o.cvhw", "--val-frac", "1.0"], capsys, "strictly between 0 and 1")
    _cli_error(["a.tfrecord"], capsys, "--output is required")


def test_fit_argument_rules_need_no_gpu():
    with pytest.raises(ValueError, match="needs validation data"):
        T._check_fit_args(None, "best")
    with pytest.raises(ValueError):
        T._check_fit_args(None, "first")
    T._check_fit_args(None, "last")
    T._check_fit_args(((), ()), "best")
