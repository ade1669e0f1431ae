"""Host side of BlobNet training (no GPU): the TFRecord reader, the sliding window, the Keras initialisation, the learning-rate
schedule and Adam step size, the dropout hash restatement, and the argument checks of covahip_train_*."""
import ctypes as C
import math

import numpy as np
import pytest

from cova_amd import _lib as L, train as T, weights as W
from cova_amd.elements import tfrecord_example
from tests import torch_blobnet_train as TT


def _frames(n, h, w, seed):
    rng = np.random.default_rng(seed)
    fr = rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    fr[..., 3] = 0
    gt = rng.integers(0, 2, (n, h, w), dtype=np.uint8)
    return fr, gt


def test_reader_round_trip_per_frame_and_gop(tmp_path):
    h, w = 5, 7
    fr, gt = _frames(6, h, w, 1)
    p1 = tmp_path / "per_frame.tfrecord"
    p1.write_bytes(b"".join(tfrecord_example(fr[i:i + 1], gt[i:i + 1]) for i in range(6)))
    f, g = T.read_tfrecords(str(p1), h, w)
    assert f.dtype == np.uint8 and g.dtype == np.uint8
    assert (f == fr).all() and (g == gt).all()
    # gop form: several strings per feature, the last record zero-filled to the GoP size
    p2 = tmp_path / "gop.tfrecord"
    p2.write_bytes(tfrecord_example(fr[:4], gt[:4], gop=4) + tfrecord_example(fr[4:], gt[4:], gop=4))
    f, g = T.read_tfrecords([str(p2)], h, w)
    assert f.shape == (8, h, w, 4) and g.shape == (8, h, w)
    assert (f[:6] == fr).all() and (g[:6] == gt).all()
    assert not f[6:].any() and not g[6:].any()
    # several files in order
    f, g = T.read_tfrecords([str(p1), str(p2)], h, w)
    assert f.shape[0] == 14 and (f[6:12] == fr).all()


def test_reader_rejects_corruption(tmp_path):
    h, w = 4, 4
    fr, gt = _frames(2, h, w, 2)
    rec = bytearray(tfrecord_example(fr, gt, gop=2))
    for pos in (9, len(rec) - 2, 20):          # length CRC, payload CRC, a payload byte
        bad = bytearray(rec)
        bad[pos] ^= 0x5A
        p = tmp_path / f"bad{pos}.tfrecord"
        p.write_bytes(bytes(bad))
        with pytest.raises(ValueError):
            T.read_tfrecords(str(p), h, w)
    for cut in (5, len(rec) - 1):
        p = tmp_path / f"cut{cut}.tfrecord"
        p.write_bytes(bytes(rec[:cut]))
        with pytest.raises(ValueError):
            T.read_tfrecords(str(p), h, w)
    p = tmp_path / "ok.tfrecord"
    p.write_bytes(bytes(rec))
    with pytest.raises(ValueError):            # wrong geometry
        T.read_tfrecords(str(p), h, w + 1)


def test_slide_order():
    h, w = 3, 2
    n = 10
    fr = np.zeros((n, h, w, 4), np.uint8)
    fr[..., 0] = np.arange(n).reshape(n, 1, 1)
    gt = np.broadcast_to(np.arange(n, dtype=np.uint8).reshape(n, 1, 1), (n, h, w)).copy()
    stacks, labels = T.slide(fr, gt)
    assert stacks.shape == (2, 4 * h, w, 4) and labels.shape == (2, h, w)
    assert [list(s[::h, 0, 0]) for s in stacks] == [[3, 2, 1, 0], [7, 6, 5, 4]]
    assert [int(l[0, 0]) for l in labels] == [3, 7]
    for s in stacks:   # row block k is one whole frame
        for k in range(4):
            assert (s[k * h:(k + 1) * h, :, 0] == s[k * h, 0, 0]).all()


def test_init_weights_keras_defaults():
    a, b = T.init_weights(7), T.init_weights(7)
    assert a.dtype == np.float32 and a.size == W.N_PARAMS and (a == b).all()
    assert not (a == T.init_weights(8)).all()
    t = W.unflatten(a)
    for name, shape in W.tensor_specs().items():
        x = t[name].astype(np.float64)
        kind = name.split(".", 1)[1]
        if kind in ("conv.kernel", "up.kernel"):
            fan_in = shape[0] * shape[1] * shape[2]       # 9 * Cin (Conv3D), 16 * Cout (Conv3DTranspose)
            std = math.sqrt(2.0 / fan_in)
            lim = 2 * std / 0.87962566103423978
            assert np.abs(x).max() <= lim * (1 + 1e-6), name
            assert abs(x.std() / std - 1) < (0.2 if x.size < 1000 else 0.05), (name, x.std(), std)
            assert abs(x.mean()) < 4 * std / math.sqrt(x.size)
        elif kind.startswith("tmix"):
            assert np.abs(x).max() <= math.sqrt(6 / 8) and x.std() > 0.2
        elif name == "final.kernel":
            assert np.abs(x).max() <= math.sqrt(6 / 17) and x.std() > 0.1
        elif kind in ("bn.gamma", "bn.var"):
            assert (x == 1).all()
        else:
            assert (x == 0).all(), name


def test_lr_schedule_and_adam_step():
    for ep in range(25):
        want = 1e-3 if ep < 10 else 1e-3 * math.exp(-0.1) ** (ep - 9)
        assert math.isclose(T.keras_lr(ep), want, rel_tol=1e-12)
    # Keras's scheduler applied epoch by epoch (lr = lr * e^-0.1 from epoch 10) gives the same numbers
    lr = 1e-3
    for ep in range(25):
        lr = lr if ep < 10 else lr * math.exp(-0.1)
        assert math.isclose(T.keras_lr(ep), lr, rel_tol=1e-12)
    # Keras Adam: lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t); one step of the update on a numpy toy problem
    g = np.array([0.5, -2.0, 1e-2])
    m = 0.1 * g
    v = 0.001 * g * g
    step = T.adam_lr_t(1e-3, 0) * m / (np.sqrt(v) + 1e-7)
    assert math.isclose(T.adam_lr_t(1e-3, 0), 1e-3 * math.sqrt(0.001) / 0.1)
    assert np.allclose(step, 1e-3 * np.sign(g), rtol=1e-3)       # the first Adam step is lr * sign(g) (for |g| >> eps)
    assert math.isclose(T.adam_lr_t(1e-3, 99), 1e-3 * math.sqrt(1 - 0.999 ** 100) / (1 - 0.9 ** 100))


def test_trainable_mask():
    mk = T.trainable_mask()
    assert mk.size == W.N_PARAMS
    n_stats = sum(int(np.prod(s)) for n, s in W.tensor_specs().items() if n.endswith((".bn.mean", ".bn.var")))
    assert (~mk).sum() == n_stats == 2 * (16 + 32 + 64 + 128 + 64 + 32 + 16)


def test_dropout_hash_restatement():
    m = TT.drop_mask(1, 0, 0, (4, 1000), 0.2)
    assert set(np.unique(m)) == {0.0, 1.25}
    assert abs((m == 0).mean() - 0.2) < 0.02
    assert (TT.drop_mask(1, 0, 0, (4, 1000), 0.2) == m).all()
    assert not (TT.drop_mask(1, 1, 0, (4, 1000), 0.2) == m).all()
    assert not (TT.drop_mask(1, 0, 1, (4, 1000), 0.2) == m).all()
    assert (TT.drop_mask(1, 0, 0, (10,), 0.0) == 1.0).all()
    # scalar and vector forms of the hash agree
    assert int(TT.splitmix64(np.array([12345], np.uint64))[0]) == TT.splitmix64(12345)


def test_default_cfg_is_the_reference_recipe():
    cfg = L.TrainCfg()
    L.lib().covahip_train_default_cfg(C.byref(cfg))
    assert (cfg.h_mb, cfg.w_mb, cfg.max_batch) == (45, 80, 4)
    assert np.float32(cfg.lr) == np.float32(1e-3) and np.float32(cfg.eps) == np.float32(1e-7)
    assert np.float32(cfg.beta1) == np.float32(0.9) and np.float32(cfg.beta2) == np.float32(0.999)
    assert np.float32(cfg.bn_momentum) == np.float32(0.99) and np.float32(cfg.bn_eps) == np.float32(1e-3)
    assert np.float32(cfg.dropout) == np.float32(0.2) and cfg.smooth == 100.0


def test_null_and_invalid_arguments_without_gpu():
    lib = L.lib()
    cfg = L.TrainCfg()
    lib.covahip_train_default_cfg(C.byref(cfg))
    lib.covahip_train_default_cfg(None)                     # no crash
    blob = W.to_bytes(T.init_weights(0))
    h = C.c_void_p(1234)
    assert lib.covahip_train_create(None, C.byref(cfg), blob, len(blob), C.byref(h)) == 1
    assert not h.value                                      # the out handle is cleared
    fake = C.c_void_p(8)                                    # never dereferenced: every check below fails first
    assert lib.covahip_train_create(fake, None, blob, len(blob), C.byref(h)) == 1
    assert lib.covahip_train_create(fake, C.byref(cfg), None, 0, C.byref(h)) == 1
    assert lib.covahip_train_create(fake, C.byref(cfg), blob, len(blob), None) == 1
    for field, value in (("h_mb", 8), ("w_mb", 2000), ("max_batch", 0), ("dropout", 1.0), ("dropout", -0.1), ("lr", -1.0),
                         ("beta1", 1.0), ("eps", 0.0), ("bn_eps", 0.0), ("bn_momentum", 1.5), ("smooth", 0.0)):
        bad = L.TrainCfg.from_buffer_copy(cfg)
        setattr(bad, field, value)
        assert lib.covahip_train_create(fake, C.byref(bad), blob, len(blob), C.byref(h)) == 1, field
    assert lib.covahip_train_create(fake, C.byref(cfg), blob[:-4], len(blob) - 4, C.byref(h)) == 6
    assert lib.covahip_train_create(fake, C.byref(cfg), b"x" * 16, 16, C.byref(h)) == 6
    loss = C.c_float()
    buf = np.zeros(16, np.uint8)
    assert lib.covahip_train_step(None, buf.ctypes.data, buf.ctypes.data, 1, 1e-3, C.byref(loss), 0) == 1
    n = C.c_size_t()
    assert lib.covahip_train_weights(None, buf.ctypes.data, 16, C.byref(n)) == 1
    g = np.zeros(W.N_PARAMS, np.float32)
    assert lib.covahip_train_grads(None, g.ctypes.data, g.size) == 1
    assert lib.covahip_train_metrics(None, (C.c_int64 * 3)()) == 1
    lib.covahip_train_destroy(None)


def test_no_gpu_creation_fails_loudly():
    lib = L.lib()
    n = C.c_int(-1)
    if lib.covahip_device_count(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("GPU host: a context can be created here; tests/test_gpu_train.py trains on it")
    h = C.c_void_p()
    assert lib.covahip_ctx_create(0, C.byref(h)) != 0 and not h.value
    cfg = L.TrainCfg()
    lib.covahip_train_default_cfg(C.byref(cfg))
    blob = W.to_bytes(T.init_weights(0))
    tr = C.c_void_p()
    assert lib.covahip_train_create(h, C.byref(cfg), blob, len(blob), C.byref(tr)) == 1   # COVAHIP_ERR_INVALID_ARG
    assert not tr.value
    from cova_amd.elements import Context
    with pytest.raises(L.CovahipError):
        Context(0)


def test_trainer_needs_a_context():
    """The Python trainer cannot reach the GPU without a context: covahip_train_create refuses a null one."""
    class NoCtx:
        handle = None

    with pytest.raises(L.CovahipError) as e:
        T.Trainer(NoCtx(), 45, 80, max_batch=4)
    assert e.value.status == 1


def test_crc32c_matches_bytewise_definition():
    assert T.crc32c(b"123456789") == 0xE3069283                 # the CRC-32C check value
    assert T.masked_crc32c(b"") == ((0 >> 15 | 0 << 17) + 0xA282EAD8) & 0xFFFFFFFF
    rng = np.random.default_rng(3)
    for n in (0, 1, 255, 2047, 2048, 2049, 14400, 70001, 1 << 20):   # the byte loop below 2 KB, the chunked form above
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        c = 0xFFFFFFFF
        for b in d:
            c ^= b
            for _ in range(8):
                c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        assert T.crc32c(d) == c ^ 0xFFFFFFFF, n
