"""CPU-only checks of Unet(dropout=p): the numpy Philox the GPU tests compare against reproduces the published known
answers, the constructor validates its argument, drop-out adds nothing to the state dict and draws nothing from torch's
RNG, and the per-rank seeds are distinct.  (That the header, the library and _hip.EXPORTS agree on the new entry points
is test_host_cpu.py's export test.)"""
import numpy as np
import pytest
import torch

import philox_ref

# Random123 kat_vectors, philox4x32 10 rounds: counter, key, output
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,out", KNOWN_ANSWERS)
def test_numpy_philox_reproduces_the_known_answers(counter, key, out):
    got = philox_ref.philox4x32_10(counter, key)
    assert tuple(int(w) for w in got) == out


def test_keep_flags_use_group_lane_step_and_site():
    """keep_flags is the known-answer generator indexed as the header states: group idx >> 2, lane idx & 3, counter words
    2 / 3 = step and site, key = the seed's halves."""
    seed, step = 0x299f31d0a4093822, 0x0370734413198a2e             # the third vector's key and counter words 2, 3
    g = (0x05a308d3 << 32) | 0x243f6a88                             # an element index has 64 bits, so a group has 62
    for site in (0, 1):
        words = philox_ref.philox4x32_10((0x243f6a88, 0x05a308d3, 0x13198a2e, 0x03707344 | (site << 31)), (0xa4093822, 0x299f31d0))
        flags = philox_ref.keep_flags(seed, step, site, 4 * g, 4, 0.5)
        assert [int(f) for f in flags] == [int(w >= 0x80000000) for w in words]
    # bit 31 of counter word 3 is the site's: the step's own bit 63 is dropped
    assert np.array_equal(philox_ref.keep_flags(seed, step | (1 << 63), 0, 4 * g, 4, 0.5), philox_ref.keep_flags(seed, step, 0, 4 * g, 4, 0.5))
    assert philox_ref.threshold(0.0) == 0 and philox_ref.threshold(0.5) == 0x80000000 and philox_ref.threshold(0.25) == 0x40000000
    assert philox_ref.threshold(np.nextafter(np.float32(1), np.float32(0))) == 0xFFFFFF00
    assert philox_ref.keep_flags(7, 3, 1, 5, 4099, 0.0).all()
    a = philox_ref.keep_flags(7, 3, 0, 0, 1 << 18, 0.5)
    assert abs(a.mean() - 0.5) < 5 * 0.5 / np.sqrt(1 << 18)
    # a window that starts inside a group is the same stream
    assert np.array_equal(philox_ref.keep_flags(7, 3, 0, 5, 100, 0.5), a[5:105])


@pytest.mark.parametrize("bad", [1.0, -0.1, 1.5, float("nan"), float("inf"), "0.5", None, True, 0.5 + 0j, [0.5]])
def test_constructor_rejects_anything_but_a_real_number_in_0_1(bad):
    import network
    with pytest.raises(ValueError, match="dropout"):
        network.check_dropout(bad)
    with pytest.raises(ValueError, match="dropout"):
        network.Unet(base_ch=32, dropout=bad)


def test_constructor_accepts_real_numbers_in_0_1():
    import network
    for ok in (0, 0.0, 0.5, np.float32(0.25), 0.999):
        assert network.check_dropout(ok) == float(ok)
    m = network.Unet(base_ch=32, dropout=0.25, dropout_seed=11)
    assert m.dropout_state() == {"p": 0.25, "seed": 11, "step": 0}
    m.load_dropout_state({"p": 0.5, "seed": 2 ** 64 - 1, "step": 9})
    assert m.dropout_state() == {"p": 0.5, "seed": 2 ** 64 - 1, "step": 9}
    with pytest.raises(ValueError):
        m.load_dropout_state({"p": 1.0, "seed": 0, "step": 0})
    with pytest.raises(ValueError):
        network.Unet(base_ch=32, dropout=0.5, dropout_seed=-1)


def test_dropout_adds_no_state_and_draws_no_parameters():
    import network
    torch.manual_seed(0)
    plain = network.Unet()
    after_plain = torch.rand(1)
    torch.manual_seed(0)
    drop = network.Unet(dropout=0.5, dropout_seed=3)
    after_drop = torch.rand(1)
    assert list(drop.state_dict().keys()) == list(plain.state_dict().keys()) and len(plain.state_dict()) == 46
    assert [k for k, _ in drop.named_buffers()] == []
    for (ka, a), (kb, b) in zip(plain.state_dict().items(), drop.state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka
    assert torch.equal(after_plain, after_drop)                      # the same number of draws from torch's generator
    assert plain.dropout == 0.0 and plain.dropout_state()["step"] == 0


def test_rank_seeds_are_distinct_and_rank_0_keeps_the_seed():
    import network
    for seed in (0, 1, 12345, 2 ** 64 - 1):
        seeds = [network.dropout_seed_for_rank(seed, r) for r in range(8)]
        assert seeds[0] == seed
        assert len(set(seeds)) == 8 and all(0 <= s < 2 ** 64 for s in seeds)
    assert network.dropout_seed_for_rank(5, 1) == 5 + 0x9E3779B97F4A7C15
    assert network.dropout_seed_for_rank(2 ** 64 - 1, 1) == 0x9E3779B97F4A7C15 - 1


def test_checkpoint_carries_the_state_only_with_dropout(tmp_path):
    """Files written for dropout = 0 keep today's keys; with dropout > 0 the state rides along and is restored."""
    import checkpoint
    import network
    import os

    class Opt:
        def state_dict(self):
            return {"state": {}, "param_groups": []}

        def load_state_dict(self, d):
            pass

    plain = network.Unet(base_ch=32)
    path = checkpoint.save_checkpoint(os.path.join(tmp_path, "plain.pth"), plain, Opt(), epoch=1)
    assert sorted(torch.load(path, weights_only=True).keys()) == ["extra", "format", "model", "optimizer"]
    drop = network.Unet(base_ch=32, dropout=0.5, dropout_seed=4)
    drop.dropout_step = 6
    path = checkpoint.save_checkpoint(os.path.join(tmp_path, "drop.pth"), drop, Opt(), epoch=1)
    assert torch.load(path, weights_only=True)["dropout"] == {"p": 0.5, "seed": 4, "step": 6}
    fresh = network.Unet(base_ch=32, dropout=0.5)
    assert checkpoint.load_checkpoint(path, fresh, Opt()) == {"epoch": 1}
    assert fresh.dropout_state() == {"p": 0.5, "seed": 4, "step": 6}
