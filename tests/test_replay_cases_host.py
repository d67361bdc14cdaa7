"""replay_cases.written / feeds / once_outputs / keep (what the launch-graph tests poison and what they leave alone) over every plan
the repository snapshots (tests/golden/plans/) and over a hand-written plan with the cases no snapshot has: a prior_box line, a
reshape alias of its output, two feeds, an output dropped behind -f32 and a +calib=.  No device."""
import importlib.util
import os

import pytest

import replay_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("dump_plans", os.path.join(ROOT, "tools", "dump_plans.py"))
dump_plans = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump_plans)
RECORDED = dump_plans.load_fixtures()


def _kernel_names(plan):
    """Kernel names as the predictor reports them, one per line, as far as keep() reads them: the device function of a prior_box
    instruction is prior_box_host_once, a reshape's reshape_share."""
    func = {"prior_box": "prior_box_host_once", "reshape": "reshape_share"}
    return ["%s -> %s" % (l.split(" ")[0], func.get(l.split("/")[0], "some_kernel_hip")) for l in plan]


def _every_output(plan):
    """(every name behind out= not dropped by -f32 and every +calib= / +hi= of the lines that are not copies to the host, the names
    dropped behind -f32), parsed on their own here."""
    outs, dropped = set(), set()
    for l in plan:
        if l.startswith("io_copy/device_to_host "):
            continue
        toks = l.split(" ")[1:]
        for t in toks:
            if t.startswith("out="):
                (dropped if "-f32" in toks else outs).update(t[4:].split(","))
            if t.startswith("+calib=") or t.startswith("+hi="):
                outs.add(t.split("=", 1)[1])
    return outs, dropped - outs


@pytest.mark.parametrize("entry", sorted(RECORDED))
def test_snapshot_plans(entry):
    plan = RECORDED[entry]
    feed_names, at = R.feeds(plan)
    assert feed_names == ["image/target_trans"] and at == [0]
    names, kept = R.to_poison(plan, _kernel_names(plan))
    assert kept == feed_names and R.once_outputs(plan) == []
    outs, dropped = _every_output(plan)
    assert set(names) == outs - set(kept) and not set(names) & dropped
    assert plan[-1].startswith("io_copy/device_to_host in=")
    fetched = plan[-1].split(" ")[1][3:]   # the program's output: the replay writes it, its host copy is not the replay's
    assert fetched in names and fetched + "/host" not in names and not [n for n in names if "," in n]
    # what the snapshots are known to hold
    if ".nofuse." in entry:
        assert not dropped and len(names) == len(plan) - 2, entry   # one variable per instruction between the two io_copy lines
    if entry.startswith("mbv3") and (".hard_act." in entry or ".all." in entry):
        assert dropped and any(n.endswith("_se_gate") for n in names), entry
    assert len(names) == len(set(names)) >= (8 if entry.startswith("two_stem") else 17)


HAND = [
    "io_copy/host_to_device in=image out=image/target_trans",
    "io_copy/host_to_device in=img_size out=img_size/target_trans",
    "reshape/def in=image/target_trans out=image_flat shape=0,-1",
    "calib/fp32_to_int8 in=image/target_trans out=image/precision_trans scale=0.00787401572",
    "conv2d/fp32_out in=image/precision_trans out=f0 +calib=f0/precision_trans scale=0.0314960629",
    "conv2d/fp32_out in=f0/precision_trans out=f1 +add=f0 +relu +calib=f1/precision_trans scale=0.0314960629 -f32",
    "prior_box/def in=f1/precision_trans,image/target_trans out=pb,pb_var min_sizes=30 max_sizes=60 aspect_ratios=2 flip=1 clip=0",
    "reshape/def in=pb out=pb_flat shape=-1,4",
    "reshape/def in=pb_flat out=pb_flat2 shape=-1,2,2",
    "reshape/def in=f0 out=f0_flat shape=0,-1",
    "split/def in=f0 out=s0,s1 axis=1 num=2",
    "shuffle_channel/unit in=s0,s1 out=lo +hi=hi +calib=hi/precision_trans scale=0.0314960629 via=cat,shuf",
    "concat/def in=pb_flat,pb_flat out=priors axis=0",
    "multiclass_nms/def in=priors,s1 out=det,det/count background=0 keep_top_k=10 normalized=1 count=det/count",
    "io_copy/device_to_host in=det/count out=det/count/host",
    "io_copy/device_to_host in=det out=det/host",
]


def test_hand_written_plan():
    plan = HAND
    assert R.feeds(plan) == (["image/target_trans", "img_size/target_trans"], [0, 1])
    assert R.once_outputs(plan) == ["pb", "pb_var", "pb_flat", "pb_flat2"]
    names, kept = R.to_poison(plan, _kernel_names(plan))
    # the feeds, prior_box's outputs, and the aliases of either (an alias of an alias too)
    assert kept == ["image/target_trans", "img_size/target_trans", "pb", "pb_var", "image_flat", "pb_flat", "pb_flat2"]
    assert len(kept) == (2 + 1) + (2 + 2)   # feeds + their alias, *_once outputs + their aliases
    assert names == sorted(["image/precision_trans", "f0", "f0/precision_trans", "f1/precision_trans", "f0_flat", "s0", "s1", "lo", "hi",
                            "hi/precision_trans", "priors", "det", "det/count"])
    assert "f1" not in names                              # dropped behind -f32
    assert "det/host" not in names and "cat" not in names  # a host copy, a via= name
    assert R.written(plan) - set(names) == set(kept)
    # a kernel that is NOT named *_once behind the same plan line: its outputs are the replay's to write
    device_prior = [k.replace("prior_box_host_once", "prior_box_hip") for k in _kernel_names(plan)]
    assert R.keep(plan, device_prior) == ["image/target_trans", "img_size/target_trans", "image_flat"]
    with pytest.raises(AssertionError):
        R.to_poison(plan, device_prior)   # the plan says host-once, the kernels say otherwise: no quiet choice
    with pytest.raises(AssertionError):
        R.keep(plan, _kernel_names(plan)[:-1])
