"""airpose_amd/_args.py: the argument rules of the data-path classes and the metric classes' base, worded once.  Every message here is
pinned character for character; the classes' own tests pin the same messages by pattern, at the place each class raises them.  No GPU:
a device with an index constructs without one, and the wrong-device tensors are stand-ins with the two attributes the rule reads."""
import types

import pytest
import torch

from airpose_amd import _args as A

NO_CPU = "%s: device must be a CUDA (ROCm) device, got cpu; there is no CPU path"


def test_device_rule():
    assert A.cuda_device("X", "cuda:1") == torch.device("cuda", 1) and A.cuda_device("X", torch.device("cuda", 0)).index == 0
    assert A.cuda_device("X", None).index is not None and A.cuda_device("X", "cuda").type == "cuda"
    with pytest.raises(RuntimeError) as e:
        A.cuda_device("X", "cpu")
    assert str(e.value) == NO_CPU % "X"


def test_the_five_classes_refuse_a_cpu_device_in_their_own_name():
    import airpose_amd
    from airpose_amd import augment, real_batches, sequence, synth_batches
    for name, make in (("RealSequenceBatches", lambda: real_batches.RealSequenceBatches(None, None, device="cpu")),
                       ("SyntheticBatches", lambda: synth_batches.SyntheticBatches(None, device="cpu")),
                       ("CropAugment", lambda: augment.CropAugment(device="cpu")),
                       ("AirPosePlusSequence", lambda: sequence.AirPosePlusSequence(None, None, device="cpu")),
                       ("CrossViewMetrics", lambda: airpose_amd.CrossViewMetrics(device="cpu"))):
        with pytest.raises(RuntimeError) as e:
            make()
        assert str(e.value) == NO_CPU % name


def test_epoch_rule():
    assert A.epoch_index("X", 0) == 0 and A.epoch_index("X", 2 ** 31 - 1) == 2 ** 31 - 1 and A.epoch_index("X", torch.tensor(7)) == 7
    with pytest.raises(RuntimeError) as e:
        A.epoch_index("X", 1.0)
    assert str(e.value) == "X: epoch must be an integer, got float"
    for bad in (-1, 2 ** 31):
        with pytest.raises(RuntimeError) as e:
            A.epoch_index("X", bad)
        assert str(e.value) == "X: epoch must be in 0 .. 2^31 - 1, got %r" % bad


def test_exact_tensor_rule():
    A.exact_tensor("X", torch.zeros(2, dtype=torch.int32), torch.int32, "index")
    with pytest.raises(RuntimeError) as e:
        A.exact_tensor("X", [1, 2], torch.int32, "index")
    assert str(e.value) == "X: index must be a tensor, got list"
    with pytest.raises(RuntimeError) as e:
        A.exact_tensor("X", torch.zeros(2, dtype=torch.float64), torch.float32, "params['gamma']")
    assert str(e.value) == "X: params['gamma'] must be float32 (nothing is cast), got torch.float64"
    with pytest.raises(RuntimeError) as e:
        A.exact_tensor("X", torch.zeros(2), torch.uint8, "frames")
    assert str(e.value) == "X: frames must be uint8 (nothing is cast), got torch.float32"


def test_lives_on_rule():
    dev = torch.device("cuda", 0)
    with pytest.raises(RuntimeError) as e:
        A.lives_on("X", torch.zeros(1), dev, "frames0", "the batches")
    assert str(e.value) == "X: frames0 lives on cpu; it must be a CUDA (ROCm) tensor, there is no CPU path"
    other = types.SimpleNamespace(is_cuda=True, device=torch.device("cuda", 1))
    for anchor in ("the batches", "the augmentation", "the fitter", "the metrics"):
        with pytest.raises(RuntimeError) as e:
            A.lives_on("X", other, dev, "z", anchor)
        assert str(e.value) == "X: z lives on cuda:1, %s on cuda:0" % anchor
    A.lives_on("X", other, None, "z", "the metrics")         # None: any CUDA device
    A.lives_on("X", other, torch.device("cuda", 1), "z", "the metrics")
