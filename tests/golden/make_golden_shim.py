"""Generate tests/golden/reference_shim.json: what the IMPORTED reference's ``models/decoder.py`` asks of ``tinycudann``.

Run once, where the reference sources are at hand (they never travel with this repository):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_shim.py <reference checkout>

The reference's ``Decoder(cfg, bound, n_class=40)`` is constructed with ``dns_slam_amd.tcnn_shim`` registered as
``tinycudann`` (INTEGRATION.md route 1).  Recorded, as plain data: every native object it builds (module path, class, the
constructor arguments of its call site), its state-dict layout (key, shape, dtype) and the derived sizes the route depends
on.  tests/test_reference_shim.py replays the recorded calls against the shim; no reference source text is stored.
"""
import json
import os
import sys
import types

import torch

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))


def main(ref_root):
    sys.path.insert(0, ROOT)
    from dns_slam_amd import synthetic, tcnn_shim

    calls = {}

    class Encoding(tcnn_shim.Encoding):
        def __init__(self, n_input_dims, encoding_config, dtype=torch.float, **kw):
            super().__init__(n_input_dims, encoding_config, dtype=dtype, **kw)
            cfg = {k: (float(v) if hasattr(v, "dtype") else v) for k, v in encoding_config.items()}    # numpy scalars -> JSON
            calls[id(self)] = ("Encoding", {"n_input_dims": int(n_input_dims), "encoding_config": cfg,
                                            "dtype": str(dtype).replace("torch.", "")})

    class Network(tcnn_shim.Network):
        def __init__(self, n_input_dims, n_output_dims, network_config, **kw):
            super().__init__(n_input_dims, n_output_dims, network_config, **kw)
            calls[id(self)] = ("Network", {"n_input_dims": int(n_input_dims), "n_output_dims": int(n_output_dims),
                                           "network_config": dict(network_config)})

    rec = types.ModuleType("tinycudann")
    rec.Encoding, rec.Network = Encoding, Network
    sys.modules["tinycudann"] = rec
    sys.path.insert(0, ref_root)
    sys.dont_write_bytecode = True                      # nothing is written next to the reference sources
    import models.decoder as ref_decoder

    bound = synthetic.load_bound(synthetic.ROOM0_BOUND)
    cfg = synthetic.default_cfg()["model"]
    ref = ref_decoder.Decoder(cfg, bound, n_class=40)
    objects = [{"path": name, "class": calls[id(mod)][0], "args": calls[id(mod)][1]}
               for name, mod in ref.named_modules() if id(mod) in calls]
    state = {k: {"shape": list(v.shape), "dtype": str(v.dtype).replace("torch.", "")} for k, v in ref.state_dict().items()}
    out = {"what": "reference models/decoder.py Decoder(cfg, room_0 bound, n_class=40) on the tinycudann shim",
           "objects": objects, "state_dict": state,
           "pe_dim": int(ref.pe_dim), "grid_dim": int(ref.grid_dim), "resolution": int(ref.pe_fn.resolution),
           "grid_total_rows": int(ref.pe_fn.grid_fn.meta.total_rows)}
    with open(os.path.join(OUT, "reference_shim.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"{len(objects)} native objects, {len(state)} state-dict entries")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_shim.py <reference checkout>")
    main(os.path.abspath(sys.argv[1]))
