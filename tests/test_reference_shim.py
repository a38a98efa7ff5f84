"""INTEGRATION.md route 1 (zero-edit): the reference's own ``models/decoder.py`` / ``models/pos_encoding.py`` constructed
against ``dns_slam_amd.tcnn_shim`` registered as ``tinycudann``.  The reference's calls into ``tinycudann`` (module path,
class and constructor arguments of every native object its ``Decoder`` builds) and the state-dict layout they produced are
stored in ``tests/golden/reference_shim.json`` (``tests/golden/make_golden_shim.py``); the test replays those calls against
the shim.  Nothing here touches a GPU: construction, constructor arguments and the state-dict layout are what the route
depends on."""
import json
import os

import pytest
import torch
from torch import nn


@pytest.fixture()
def reference_calls(golden_dir):
    with open(os.path.join(golden_dir, "reference_shim.json")) as f:
        return json.load(f)


def _replay(calls):
    """A module tree with the shim's objects at the reference's module paths, built from the reference's recorded calls."""
    from dns_slam_amd import tcnn_shim
    root = nn.Module()
    for obj in calls["objects"]:
        args = dict(obj["args"])
        if obj["class"] == "Encoding":
            args["dtype"] = getattr(torch, args["dtype"])
        mod = getattr(tcnn_shim, obj["class"])(**args)
        *parents, leaf = obj["path"].split(".")
        node = root
        for p in parents:
            if not hasattr(node, p):
                node.add_module(p, nn.Module())
            node = getattr(node, p)
        node.add_module(leaf, mod)
    return root


def test_reference_decoder_constructs_on_the_shim(reference_calls):
    from dns_slam_amd import synthetic
    from dns_slam_amd.decoder import Decoder
    from dns_slam_amd import tcnn_shim
    bound = synthetic.load_bound(synthetic.ROOM0_BOUND)
    cfg = synthetic.default_cfg()["model"]
    ref = _replay(reference_calls)
    own = Decoder(cfg, bound, n_class=40)
    sd_ref, sd_own = ref.state_dict(), own.state_dict()
    assert set(sd_ref) == set(sd_own) == set(reference_calls["state_dict"]) == {
        "pe_fn.grid_fn.params", "pe_fn.pe_fn.params", "coarse_fn.decoder.params", "out_fn.color_decoder.params",
        "out_fn.logit_decoder.params", "merge.decoder.params", "merge.pe_fn.params"}
    for k in sd_ref:
        want = reference_calls["state_dict"][k]
        assert list(sd_ref[k].shape) == list(sd_own[k].shape) == want["shape"], k
        assert sd_ref[k].dtype == torch.float32 and want["dtype"] == "float32", k
    # every native object the reference built is the shim's, with the constructor arguments of the cited call sites
    assert isinstance(ref.coarse_fn.decoder, tcnn_shim.Network) and isinstance(ref.pe_fn.grid_fn, tcnn_shim.Encoding)
    assert (ref.coarse_fn.decoder.n_input_dims, ref.coarse_fn.decoder.n_output_dims) == (80, 33)      # decoder.py:84
    assert (ref.out_fn.color_decoder.n_input_dims, ref.out_fn.color_decoder.n_output_dims) == (112, 3)  # decoder.py:101
    assert ref.out_fn.logit_decoder.n_output_dims == 40                                                 # decoder.py:110
    assert ref.merge.decoder.n_input_dims == 112 and ref.merge.decoder.n_output_dims == 32              # decoder.py:58
    assert ref.pe_fn.pe_fn.n_output_dims == reference_calls["pe_dim"] == own.pe_dim == 48
    assert ref.pe_fn.grid_fn.n_output_dims == reference_calls["grid_dim"] == own.grid_dim == 32
    assert reference_calls["resolution"] == own.pe_fn.resolution == 592
    assert ref.pe_fn.grid_fn.meta.total_rows == reference_calls["grid_total_rows"] == 853312                # room_0 table
    # a state dict written by one loads into the other (checkpoint interop at the module level)
    own.load_state_dict(sd_ref)
    ref.load_state_dict(sd_own)
