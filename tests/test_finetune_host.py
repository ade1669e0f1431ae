"""Host side of fine-tuning (cova_amd/train.py, no GPU): plan names <-> bits, the CLI's --init / --freeze / --freeze-bn rules and
the --init directory of a set."""
import ctypes as C

import pytest

from cova_amd import _lib as L
from cova_amd import train as T


def test_names_and_bits():
    assert T.GROUPS == ("enc0", "enc1", "enc2", "enc3", "dec0", "dec1", "dec2", "dec3") and T.BN_LAYERS == T.GROUPS[:7]
    assert T.plan_bits() == (0, 0)
    for k, name in enumerate(T.GROUPS):
        assert T.plan_bits(freeze=(name,)) == (1 << k, 0)
        assert T.plan_bits(freeze=name) == (1 << k, 0)
    for k, name in enumerate(T.BN_LAYERS):
        assert T.plan_bits(bn_inference=(name,)) == (0, 1 << k)
    assert T.plan_bits(freeze="encoder") == (0x0F, 0)
    assert T.plan_bits(freeze="decoder") == (0xF0, 0)
    assert T.plan_bits(freeze="enc0,enc2,dec1") == (0b0010_0101, 0)
    assert T.plan_bits(freeze=["enc1", "enc1", "encoder"]) == (0x0F, 0)                 # duplicates are one bit
    assert T.plan_bits(bn_inference="all") == (0, 0x7F)
    assert T.plan_bits(bn_inference="encoder") == (0, 0x0F)
    assert T.plan_bits(bn_inference="decoder") == (0, 0x70)                             # dec3 has no BatchNorm
    assert T.plan_bits(freeze=("encoder", "dec0", "dec1", "dec2"), bn_inference=("dec0",)) == (0x7F, 0x10)
    # the bits given, not the effective ones: the library adds the frozen groups' layers
    assert T.plan_bits(freeze="enc2") == (4, 0)
    for bad in (dict(freeze="enc4"), dict(freeze=("dec", )), dict(freeze="all"), dict(bn_inference="dec3"), dict(bn_inference=("bn0",)),
                dict(freeze="encoder,decoder"), dict(freeze=T.GROUPS)):
        with pytest.raises(ValueError):
            T.plan_bits(**bad)
    assert T.plan_names(0, 0) == {"freeze": (), "bn_inference": ()}
    assert T.plan_names(0b0001_0100, 0b0001_0101) == {"freeze": ("enc2", "dec0"), "bn_inference": ("enc0", "enc2", "dec0")}
    for fz in (0, 1, 0x0F, 0xF0, 0x7F, 0xA5):
        names = T.plan_names(fz, fz & 0x7F)
        assert T.plan_bits(names["freeze"], names["bn_inference"]) == (fz, fz & 0x7F)


def test_plan_structure_layout():
    assert C.sizeof(L.TrainPlan) == 8
    assert [f[0] for f in L.TrainPlan._fields_] == ["frozen_groups", "bn_inference"]
    p = L.TrainPlan(0x12, 0x34)
    assert bytes(p) == bytes([0x12, 0, 0, 0, 0x34, 0, 0, 0])
    for name in ("covahip_train_set_plan", "covahip_train_get_plan"):
        assert name in L.PROTOTYPES


def _cli_error(argv, capsys, text):
    with pytest.raises(SystemExit) as e:
        T.parse_args(argv)
    assert e.value.code == 2
    assert text in capsys.readouterr().err


def test_cli_argument_rules(capsys):
    a = T.parse_args(["a.tfrecord", "-o", "o.cvhw"])
    assert a.init is None and a.freeze is None and not a.freeze_bn
    assert T._plan_kw(a) == {"freeze": (), "bn_inference": ()}
    a = T.parse_args(["a.tfrecord", "-o", "o.cvhw", "--init", "base.cvhw", "--freeze", "encoder", "--freeze-bn"])
    assert a.init == "base.cvhw" and T._plan_kw(a) == {"freeze": "encoder", "bn_inference": "all"}
    assert T.plan_bits(**T._plan_kw(a)) == (0x0F, 0x7F)
    a = T.parse_args(["a.tfrecord", "-o", "o.cvhw", "--freeze", "enc0,enc1,dec3", "--resume", "run.cvhs"])    # resume keeps its flags
    assert T.plan_bits(**T._plan_kw(a)) == (0x83, 0)
    a = T.parse_args(["--set", "-o", "dir", "a.tfrecord", "b.tfrecord", "--init", "bases", "--freeze", "decoder"])
    assert a.as_set and a.init == "bases"
    _cli_error(["a.tfrecord", "-o", "o.cvhw", "--init", "base.cvhw", "--resume", "run.cvhs"], capsys, "--init and --resume exclude each other")
    _cli_error(["a.tfrecord", "-o", "o.cvhw", "--freeze", "enc0,enc9"], capsys, "unknown name 'enc9'")
    _cli_error(["a.tfrecord", "-o", "o.cvhw", "--freeze", "encoder,decoder"], capsys, "nothing left to train")
    _cli_error(["a.tfrecord", "-o", "o.cvhw", "--freeze", "enc0,enc1,enc2,enc3,dec0,dec1,dec2,dec3"], capsys, "nothing left to train")
    _cli_error(["--eval-only", "w.cvhw", "a.tfrecord", "--freeze", "encoder"], capsys, "--eval-only trains nothing")
    _cli_error(["--eval-only", "w.cvhw", "a.tfrecord", "--init", "w.cvhw"], capsys, "--eval-only trains nothing")


def test_init_paths_of_a_set(tmp_path):
    records = ["data/cam0.tfrecord", "cam1.tfrecord", "x/cam2a.tfrecord,x/cam2b.tfrecord"]
    one = tmp_path / "base.cvhw"
    one.write_bytes(b"")
    assert T.init_paths(records, str(one)) == [str(one)] * 3                               # one file for every model
    d = tmp_path / "bases"
    d.mkdir()
    for stem in ("cam0", "cam1"):
        (d / f"{stem}.cvhw").write_bytes(b"")
    with pytest.raises(ValueError, match="cam2a.cvhw"):                                    # named as --set -o names them
        T.init_paths(records, str(d))
    (d / "cam2a.cvhw").write_bytes(b"")
    assert T.init_paths(records, str(d)) == [str(d / f"{s}.cvhw") for s in ("cam0", "cam1", "cam2a")]
    assert T.init_paths(records, str(d)) == [p for _, p in T.set_jobs(records, str(d))]
