"""tools/eval_device.py's host pieces on the CPU: the --switch parser and the actor loader (fc1..fc4 out of a MADDPG
checkpoint dict, without importing the reference)."""
import importlib.util
import os

import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("eval_device", os.path.join(ROOT, "tools", "eval_device.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_parse_switch(tool):
    assert tool.parse_switch("0:4,300:5") == {0: 4, 300: 5}
    assert tool.parse_switch("") == {} and tool.parse_switch(None) == {} and tool.parse_switch("7:0,") == {7: 0}
    with pytest.raises(ValueError):
        tool.parse_switch("3")


def test_load_actor_reads_fc1_to_fc4(tool, tmp_path):
    from marl_llm_amd.rollout import PolicyMLP
    torch.manual_seed(1)
    actor = PolicyMLP(192, 2, 180)
    sd = {"module." + k: v for k, v in actor.state_dict().items()}           # a prefixed state dict, as a wrapped module saves
    ckpts = {"maddpg.pt": {"init_dict": {"hidden_dim": 180}, "agent_params": [{"policy": actor.state_dict(), "critic": {}}]},
             "agent.pt": {"policy": sd}, "bare.pt": actor.state_dict()}
    for name, ckpt in ckpts.items():
        path = str(tmp_path / name)
        torch.save(ckpt, path)
        got = tool.load_actor(path)
        assert isinstance(got, PolicyMLP)
        assert all(torch.equal(a, b) for a, b in zip(actor.state_dict().values(), got.state_dict().values())), name
    bad = actor.state_dict()
    del bad["fc3.bias"]
    torch.save(bad, str(tmp_path / "bad.pt"))
    with pytest.raises(KeyError, match="fc3.bias"):
        tool.load_actor(str(tmp_path / "bad.pt"))
