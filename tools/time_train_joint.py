#!/usr/bin/env python3
"""Time one posterior-joint-training step (joint_posterior_loss: fixed-T decode with the per-iteration loss and its
posterior-local HIP gradients, backward scaling, Adam) next to the existing full-backpropagation step (forward with saved
messages, HIP backward sweeps, Adam) at the same size.

    python tools/time_train_joint.py [--steps 10] [--decoder neural2d|wrcq|layered|wrcq_layered]
Prints one JSON line with a result per workload: (1998,1512) Neural-2D type 2 at T = 10 with B = 4096 and 32768, and
(16200,7200) at T = 20 with B = 1024.  Device events around each step.  Algorithmic HBM bytes of a PJT step, per codeword
and iteration: forward sweeps 16E + 8n (check: read v2c, write c2v; variable: read c2v + llr, write v2c + posterior), loss
8n (read posterior, write g_l), local backward 20E (check: read v2c, gathered g_l and write d/dv2c; variable: read c2v_t-1
and d/dv2c).
--decoder wrcq times the same step of the quantised WeightedRCQDecoder (type 2, bc = 3, three quantisers,
quantizer_gradient="straight_through") on the same workloads; it has no full-backpropagation step to stand next to.  Its
C2V rows are 1-byte codes: forward sweeps 10E + 8n, loss 8n, local backward 18E (check: v2c, codes, gathered g_l, write
d/dv2c; variable: codes of t-1 and d/dv2c) -- 28E + 16n against 36E + 16n.
--decoder layered times the step of Neural2DMinSumDecoder(schedule="layered", layered_gradient="posterior_local") on the
same workloads (no full-backpropagation step exists for it) and, beside it, the forward alone (the one-wave-per-tile walk
and the per-iteration loss, no gradient kernels: engine.train_joint_layered(want_grads=False)) -- `forward_share` is that
time over the step's.  Algorithmic bytes: walk 28E (two passes reading P and R, the second writing P, R and u), posterior
copy and loss 16n, check backward 12E (u, gathered g_l, write d/du) -- 40E + 16n.
--decoder wrcq_layered times the step of WeightedRCQDecoder(layered="paper", quantizer_gradient="straight_through",
layered_gradient="posterior_local") (type 2, bc = 3, three quantisers) on the same workloads, with `forward_share` as for
--decoder layered (engine.train_joint_layered_ste(want_grads=False)).  Algorithmic bytes: walk 14E (the held form: one read
of P and of the 1-byte codes, writing P, codes and u), posterior copy and loss 16n, check backward 13E (u, codes, gathered
g_l, write d/du) -- 27E + 16n.
--learn-quantizer (with --decoder wrcq or wrcq_layered) adds the same step of the decoder built with learn_quantizer=True --
the level gradient (kernel level_grad: E code bytes and 4E gathered seed bytes per codeword and iteration on top of the
step's bytes), the chain rule to (C, gamma), Adam on the float64 pair and the re-upload of the moved thresholds into the same
native decoder (DecodeEngine.set_quantizers) -- as `levels_ms_per_step`, and the engine call alone with and without
grad_levels (engine.train_joint_ste(want_levels=...), no autograd, no optimiser) as `engine_ms` / `engine_levels_ms`;
`levels_bytes_ratio` is 5E over the step's algorithmic bytes, the overhead the added traffic alone would cost."""
import argparse, json, os, sys
os.environ.setdefault("LDPC_TRAIN_MAX_SAVED_BYTES", str(64 << 30))     # let the BPTT step run where the HBM holds it
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (puts the package on sys.path)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

WORKLOADS = (("ira_1998_1512", 10, 4096), ("ira_1998_1512", 10, 32768), ("dvbs2_like_16200_7200", 20, 1024))


def time_steps(step, steps):
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    e0, e1 = ev(), ev()
    e0.record()
    for _ in range(steps):
        loss = step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps, float(loss.item())


WRCQ_QUANTIZERS = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]


def run(name, T, B, steps, snr_db, dev, decoder="neural2d", learn_quantizer=False):
    import autograd_bridge as ab
    import codes
    from neural_2d_decoder import Neural2DMinSumDecoder
    from rcq_decoder import WeightedRCQDecoder
    code = codes.load_code(name, max_iterations=T)
    wrcq, layered, wrcq_lay = decoder == "wrcq", decoder == "layered", decoder == "wrcq_layered"
    model = (WeightedRCQDecoder(code, 3, 8, WRCQ_QUANTIZERS, 2, T, quantizer_gradient="straight_through") if wrcq
             else WeightedRCQDecoder(code, 3, 8, WRCQ_QUANTIZERS, 2, T, layered="paper", quantizer_gradient="straight_through",
                                     layered_gradient="posterior_local") if wrcq_lay
             else Neural2DMinSumDecoder(code, 2, T, schedule="layered", layered_gradient="posterior_local") if layered
             else Neural2DMinSumDecoder(code, 2, T))
    with torch.no_grad():
        for p in model.beta_weights.values():
            p.fill_(0.7)
        for p in model.alpha_weights.values():
            p.fill_(1.0)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    llr = bench.make_llr(B, code.n, snr_db, 1234, dev)
    tgt = torch.zeros_like(llr)
    g = code.tanner_graph()

    def pjt():
        opt.zero_grad()
        loss = model.joint_posterior_loss(llr)[0]
        loss.backward()
        opt.step()
        return loss

    def bptt():
        opt.zero_grad()
        _, post, _ = model(llr, early_stop=False)
        loss = F.binary_cross_entropy_with_logits(-post, tgt)
        loss.backward()
        opt.step()
        return loss

    eng = model._get_engine(dev)
    ms, loss = time_steps(pjt, steps)
    alg = B * T * ((28 if wrcq else 40 if layered else 27 if wrcq_lay else 36) * g.E + 16 * g.n)
    ws = (eng.train_joint_ste_workspace_bytes(B) if wrcq else eng.train_joint_layered_workspace_bytes(B) if layered
          else eng.train_joint_layered_ste_workspace_bytes(B) if wrcq_lay else eng.train_joint_workspace_bytes(B))
    label = "W-RCQ bc=3" if wrcq else "layered Neural2D" if layered else "layered W-RCQ bc=3" if wrcq_lay else "Neural2D"
    out = {"workload": f"{name} {label} type 2, T={T}, batch {B}", "pjt_ms_per_step": ms,
           "pjt_codewords_per_s": B / ms * 1e3, "pjt_algorithmic_GBps": alg / (ms * 1e-3) / 1e9,
           "pjt_workspace_bytes_per_codeword": ws / B, "pjt_loss": loss}
    if layered or wrcq_lay:                                # the forward alone: the walk and the loss, no gradient kernels
        forward = eng.train_joint_layered if layered else eng.train_joint_layered_ste

        def forward_only():
            return forward(llr, want_grads=False)["loss"]
        ms_f, _ = time_steps(forward_only, steps)
        out.update({"forward_ms_per_step": ms_f, "forward_share": ms_f / ms})
    if learn_quantizer and (wrcq or wrcq_lay):
        call = eng.train_joint_ste if wrcq else eng.train_joint_layered_ste
        ms_e, _ = time_steps(lambda: call(llr, want_grad_llr=False)["loss"], steps)
        ms_l, _ = time_steps(lambda: call(llr, want_grad_llr=False, want_levels=True)["loss"], steps)
        how = dict(quantizer_gradient="straight_through", learn_quantizer=True)
        if wrcq_lay:
            how.update(layered="paper", layered_gradient="posterior_local")
        learn = WeightedRCQDecoder(code, 3, 8, WRCQ_QUANTIZERS, 2, T, **how)
        learn.load_state_dict(model.state_dict(), strict=False)
        opt_l = torch.optim.Adam(learn.parameters(), lr=1e-3)

        def pjt_levels():
            opt_l.zero_grad()
            loss = learn.joint_posterior_loss(llr)[0]
            loss.backward()
            opt_l.step()
            return loss

        ms_s, loss_s = time_steps(pjt_levels, steps)
        eng_l = learn._get_engine(dev)
        ws_l = int(getattr(eng_l._lib, "ldpc_train_joint_ste_levels_workspace_bytes" if wrcq
                           else "ldpc_train_joint_layered_ste_levels_workspace_bytes")(eng_l.handle, B))
        out.update({"engine_ms": ms_e, "engine_levels_ms": ms_l, "engine_levels_overhead": ms_l / ms_e - 1.0,
                    "levels_ms_per_step": ms_s, "levels_step_overhead": ms_s / ms - 1.0, "levels_loss": loss_s,
                    "levels_bytes_ratio": 5 * g.E / ((28 if wrcq else 27) * g.E + 16 * g.n),
                    "levels_workspace_bytes_per_codeword": ws_l / B,
                    "learned": [[float(c), float(gm)] for c, gm in zip(learn.quantizer_C.tolist(), learn.quantizer_gamma.tolist())]})
        del learn, opt_l, eng_l
    if wrcq or layered or wrcq_lay:                        # no saved-history path exists for these decoders
        del model, opt, eng
        torch.cuda.empty_cache()
        return out
    saved = eng.train_saved_bytes(B)
    out["bptt_saved_bytes_per_codeword"] = saved / B
    if saved <= ab.MAX_SAVED_BYTES:
        torch.cuda.empty_cache()
        ms_b, loss_b = time_steps(bptt, steps)
        out.update({"bptt_ms_per_step": ms_b, "bptt_codewords_per_s": B / ms_b * 1e3, "bptt_loss": loss_b,
                    "pjt_over_bptt_time": ms / ms_b})
    else:
        out["bptt_ms_per_step"] = None                     # the saved history does not fit the cap
    del model, opt, eng
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--snr-db", type=float, default=3.0)
    ap.add_argument("--workload", type=int, default=None, help="run only WORKLOADS[i]")
    ap.add_argument("--decoder", choices=("neural2d", "wrcq", "layered", "wrcq_layered"), default="neural2d")
    ap.add_argument("--learn-quantizer", action="store_true", help="also time the step with the level gradient (wrcq, wrcq_layered)")
    a = ap.parse_args()
    if a.learn_quantizer and a.decoder not in ("wrcq", "wrcq_layered"):
        ap.error("--learn-quantizer needs --decoder wrcq or wrcq_layered")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    todo = WORKLOADS if a.workload is None else WORKLOADS[a.workload:a.workload + 1]
    res = [run(name, T, B, a.steps, a.snr_db, dev, a.decoder, a.learn_quantizer) for name, T, B in todo]
    print(json.dumps({"tool": "time_train_joint", "decoder": a.decoder, "learn_quantizer": a.learn_quantizer, "steps": a.steps,
                      "results": res}))


if __name__ == "__main__":
    main()
