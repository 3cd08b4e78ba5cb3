"""CPU-side checks of GpuImageLoader's one iteration body: for 63 option sets, at both ``return_index`` settings, what the loader hands to its
transform and what it yields.  The expectation of every record kind comes from the documented drawing order (the plan, then augment words or
crop windows, mix, erase, colour, blur records; ``three_augment`` draws colour and blur together) applied to a fresh generator of the same seed,
never from the loader.  A recording stand-in is the transform, so nothing here needs a GPU."""
import itertools

import numpy as np
import pytest
import torch

import qat_vit_amd

N, BATCH, SEED, OUT = 20, 8, 12, 36


class _Recorder:
    """A stand-in transform: keeps what the loader hands to every call."""
    device, out_size = torch.device("cpu"), OUT

    def __init__(self):
        self.calls = []

    def __call__(self, images, index, **kw):
        self.calls.append({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in dict(kw, index=index).items()})
        return torch.zeros(index.shape[0], 3, 1, 1)


def _option_sets():
    fronts = {"none": {}, "augment": {"augment": qat_vit_amd.RandomCropFlip(2, padding_mode="reflect")}, "crop": {"crop": qat_vit_amd.RandomResizedCrop()}}
    late = {"mix": qat_vit_amd.MixupCutmix(mode="elem"), "erase": qat_vit_amd.RandomErasing(p=0.6),
            "color": qat_vit_amd.ColorJitter(0.4, 0.4, 0.4, grayscale=0.2), "blur": qat_vit_amd.GaussianBlur(p=0.5)}
    subsets = lambda names: [c for k in range(len(names) + 1) for c in itertools.combinations(names, k)]   # noqa: E731
    tails = [{k: late[k] for k in c} for c in subsets(("mix", "erase", "color", "blur"))]
    tails += [dict({k: late[k] for k in c}, three_augment=qat_vit_amd.ThreeAugment()) for c in subsets(("mix", "erase"))]
    tails.append({"color": qat_vit_amd.ColorJitter(0.4, 0, 0.4)})
    return [("-".join([f] + list(t)), dict(front, **t)) for f, front in fronts.items() for t in tails]


SETS = _option_sets()


def test_the_option_sets_are_the_sixty_three():
    assert len(SETS) == 3 * (16 + 4 + 1) == 63                       # per front: the subsets of four, three_augment with the subsets of two, no contrast


def _expected(opts):
    """(plan, {keyword: the epoch's records}) of the documented drawing order, from a fresh generator."""
    g = torch.Generator().manual_seed(SEED)
    plan = qat_vit_amd.epoch_batches(N, BATCH, shuffle=True, generator=g)
    want = {}
    if "augment" in opts:
        want["aug"] = opts["augment"].draw(N, g)
    if "crop" in opts:
        want["rrc"] = opts["crop"].draw(N, 8, g)
    if "mix" in opts:
        want["mix"] = opts["mix"].draw([len(p) for p in plan], OUT, g)
    if "erase" in opts:
        want["erase"] = opts["erase"].draw(N, OUT, g)
    if "color" in opts:
        want["color"] = opts["color"].draw(N, g)
    if "blur" in opts:
        want["blur"] = opts["blur"].draw(N, g)
    if "three_augment" in opts:
        want["color"], want["blur"] = opts["three_augment"].draw(N, g)
    return plan, want


@pytest.mark.parametrize("return_index", [False, True], ids=["plain", "index"])
@pytest.mark.parametrize("opts", [o for _, o in SETS], ids=[f"{i:02d}-{name}" for i, (name, _) in enumerate(SETS)])
def test_calls_and_tuples_follow_the_documented_order(monkeypatch, opts, return_index):
    empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, pin_memory=False, **k: empty(*a, **k))       # no accelerator here: the block is not pinned
    rng = np.random.default_rng(3)
    imgs, labels = rng.integers(0, 256, (N, 8, 8, 3), dtype=np.uint8), rng.integers(0, 10, N)
    tr = _Recorder()
    loader = qat_vit_amd.GpuImageLoader(imgs, labels, BATCH, shuffle=True, generator=torch.Generator().manual_seed(SEED), transform=tr,
                                        return_index=return_index, **opts)
    tuples = list(loader)
    plan, want = _expected(opts)
    calls = tr.calls
    assert len(calls) == len(tuples) == len(plan) == 3
    assert torch.equal(torch.cat([c["index"] for c in calls]), torch.cat(plan))
    for c, p in zip(calls, plan):                                    # every call is sliced at the plan's batch boundaries
        assert torch.equal(c["index"], p)
        for key in want:
            assert c[key].dtype == torch.int32 and c[key].shape[0] == len(p), key
    for key in ("aug", "rrc", "mix", "erase", "color", "blur"):
        if key in want:
            assert torch.equal(torch.cat([c[key] for c in calls]), want[key]), key
        else:
            assert all(c.get(key) is None for c in calls), key       # an absent keyword counts as None
    a = opts.get("augment")
    for c in calls:
        if a is not None:
            assert (c["padding_mode"], c["fill"], c["padding"]) == (a.padding_mode, a.fill, a.padding) == ("reflect", 0, 2)
        else:
            assert not {"padding_mode", "fill", "padding"} & set(c)
        jitter = opts.get("color", opts.get("three_augment"))
        if jitter is not None:
            assert c["contrast"] is (jitter.contrast is not None)
        else:
            assert not c.get("contrast")
    if not opts:
        assert all(set(c) == {"index"} for c in calls)               # no option: transform(data, idx), no keyword at all
    dev_labels = torch.as_tensor(labels)
    for t, c in zip(tuples, calls):
        assert len(t) == 2 + return_index + ("mix" in opts)
        assert tuple(t[0].shape) == (len(c["index"]), 3, 1, 1) and torch.equal(t[1], dev_labels[c["index"]])
        if return_index:
            assert torch.equal(t[2], c["index"])
        if "mix" in opts:
            assert torch.equal(t[-1], c["mix"])


def test_a_loader_without_options_takes_any_callable(monkeypatch):
    empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, pin_memory=False, **k: empty(*a, **k))

    class Foreign:                                                   # no out_size, and no keyword in its signature
        device = torch.device("cpu")

        def __call__(self, images, index):
            return images[index]

    imgs = np.arange(5 * 8 * 8 * 3, dtype=np.uint8).reshape(5, 8, 8, 3)
    out = list(qat_vit_amd.GpuImageLoader(imgs, np.arange(5), 2, transform=Foreign()))
    assert [tuple(x.shape) for x, _ in out] == [(2, 8, 8, 3), (2, 8, 8, 3), (1, 8, 8, 3)] and torch.equal(torch.cat([y for _, y in out]), torch.arange(5))
