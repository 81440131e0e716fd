"""Golden of the fp64 multi-network closure from the UNMODIFIED reference under its float64 defaults: c1_f64 -- the C1 system
(Lotka-Volterra on two FCNN(1, 1, (32, 32), SinActv)) at 64 points, run the way an unchanged reference script runs it: networks
initialised in double, points drawn in double, one closure and a 3-epoch Adam trajectory of the reference solver in double.  Run
where the reference is installed, next to make_golden.py, whose config, closure and parameter helpers this reuses unchanged
(its ``make_default_precision`` is the same recipe for the 2-D solver).  Writes data only."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the reference on sys.path and imports it)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def make(name="c1_f64", base="c1", seed=0):
    MG.set_tensor_type(device="cpu", float_bits=64)
    try:
        torch.manual_seed(seed)
        cfg = MG.CONFIGS[base]()
        gen = cfg["gen"]
        torch.manual_seed(seed + 1)
        draw = gen.get_examples()
        coords = [d.detach().clone() for d in ([draw] if isinstance(draw, torch.Tensor) else list(draw))]
        assert coords[0].dtype == torch.float64 and next(cfg["nets"][0].parameters()).dtype == torch.float64
        out = dict(seed=np.asarray(seed), params0=MG.flat_params(cfg["nets"]).numpy(), coords=np.stack([c.numpy() for c in coords]))
        keep = [{k: v.clone() for k, v in n.state_dict().items()} for n in cfg["nets"]]
        for k, v in MG.closure_once(cfg, coords, torch.float64).items():
            out[f"{k}_f64"] = v
        for n, sd in zip(cfg["nets"], keep):   # (closure_once hands the networks back in fp32: restore the double weights exactly)
            n.double()
            n.load_state_dict(sd)
        assert np.array_equal(MG.flat_params(cfg["nets"]).numpy(), out["params0"])
        solver = MG.Solver1D(cfg["pde"], cfg["conds"], nets=cfg["nets"], train_generator=gen, valid_generator=gen, n_batches_valid=0,
                             t_min=0.1, t_max=12.0)
        torch.manual_seed(seed + 2)
        for _ in range(3):
            solver.run_train_epoch()
        out["traj_loss"] = np.asarray(solver.metrics_history["train_loss"])
        out["traj_params"] = MG.flat_params(cfg["nets"]).numpy()
        assert out["traj_params"].dtype == np.float64
    finally:
        MG.set_tensor_type(device="cpu", float_bits=32)
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(name, "(float64 defaults) N =", coords[0].numel(), "loss64 =", float(out["loss_f64"]), "traj =", out["traj_loss"], "->",
          os.path.getsize(path), "bytes")


if __name__ == "__main__":
    make()
