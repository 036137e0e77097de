"""
Drop-in for the reference module of the same name (neural_minsum_decoder.py): the original
neural MinSum decoders with one weight per (iteration, edge), ``forward`` on the MI355X engine
(they fall out of the same kernels with a per-edge weight table).

Reference behaviour mirrored (file:line in /root/reference):
  NeuralMinSumDecoder(code, max_iterations=50)             neural_minsum_decoder.py:19-150
      beta_weights["iter_{t}_c{i}_v{j}"], init randn*0.1 + 0.7, created iteration-major then in
      row-major edge order (so equal seeds give equal weights);
      C2V = beta * min * prod(signs); V2C = llr + sum(others); -> (int32[n], float32[n], int)
  NeuralOffsetMinSumDecoder(code, max_iterations=50)       neural_minsum_decoder.py:152-286
      init randn*0.1; C2V = prod(signs) * relu(min - beta)
  analyze_weight_patterns(decoder, code)                   neural_minsum_decoder.py:288-349

Extensions as everywhere: ``[B, n]`` batches, ``early_stop=False``; keyword-only ``schedule="layered"`` runs the layered
schedule with the per-edge weights (ldpc_decoder.py module docstring; ``forward`` with autograd on raises
NotImplementedError, and so does ``joint_posterior_loss`` unless ``layered_gradient="posterior_local"`` -- constructor
argument, or keyword of ``joint_posterior_loss`` -- asks for the layered posterior-local gradient of include/ldpc_hip.h).
"""

from __future__ import annotations

import logging
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from ldpc_decoder import LDPCCode, _as_batch, check_schedule

logger = logging.getLogger(__name__)


class _EdgeWeightDecoder(nn.Module):
    """one beta per (iteration, edge); table column = CSR edge id"""

    _c2v_form = "nms"
    schedule = "flooding"          # "layered": the layered schedule (ldpc_decoder.py module docstring)
    layered_gradient = None        # "posterior_local": joint_posterior_loss of a layered decoder trains with that gradient

    def _refuse_layered_grad(self, what: str):
        if self.schedule == "layered":
            raise NotImplementedError(f"{type(self).__name__}(schedule=\"layered\") has no gradient path: {what} exists "
                                      "for the flooding schedule only (joint_posterior_loss trains a layered decoder "
                                      "with layered_gradient=\"posterior_local\")")

    def _init_edges(self, code: LDPCCode, max_iterations: int, offset: float):
        self.code = code
        self.max_iterations = max_iterations
        g = code.tanner_graph()
        self.beta_weights = nn.ParameterDict()
        rows, cols = g.check_of_edge.tolist(), g.var_idx.tolist()      # row-major == the reference's i, j loops
        for t in range(max_iterations):
            for i, j in zip(rows, cols):
                w = torch.randn(1) * 0.1
                if offset:
                    w = w + offset
                self.beta_weights[f"iter_{t}_c{i}_v{j}"] = nn.Parameter(w)
        self._engine = None
        self._engine_key = None
        self._uploaded: Optional[np.ndarray] = None
        self._cells = None

    def __getstate__(self):
        state = self.__dict__.copy()
        state.update(_engine=None, _engine_key=None, _uploaded=None, _cells=None)
        return state

    def weight_table(self) -> np.ndarray:
        """beta[T, E] float32 in CSR edge order (KeyError for a missing key, like the reference).  WHICH parameter feeds
        which cell is resolved once per parameter set; the VALUES are read on every call."""
        g = self.code.tanner_graph()
        T = int(self.max_iterations)
        out = np.zeros((max(T, 1), max(g.E, 1)), dtype=np.float32)
        if T and g.E:
            who = (tuple(map(id, self.beta_weights.values())), T, id(g))
            if self._cells is None or self._cells[0] != who:
                rows, cols = g.check_of_edge.tolist(), g.var_idx.tolist()
                self._cells = (who, [self.beta_weights[f"iter_{t}_c{i}_v{j}"] for t in range(T) for i, j in zip(rows, cols)])
            params = self._cells[1]
            out[:T, :g.E] = torch.cat([p.detach().reshape(-1)[:1] for p in params]).to("cpu", torch.float32) \
                .numpy().reshape(T, g.E)
        return out

    def _get_engine(self, device):
        import _native as nat
        from engine import DecodeEngine, _require_gpu
        dev = _require_gpu(device)
        g = self.code.tanner_graph()
        T = int(self.max_iterations)
        key = (dev.index, id(g), T, self.schedule)
        # flattened on every call and compared with the last upload by value: a write through `p.data` moves no version
        # counter (neural_2d_decoder.py, _get_engine)
        beta = self.weight_table()
        if self._engine is None or self._engine_key != key:
            rows = max(T, 1)
            extra = {"schedule": nat.SCHED_LAYERED} if self.schedule == "layered" else {}
            self._engine = DecodeEngine(
                g, dtype=torch.float32, iters=T, device=dev,
                c2v_form=nat.C2V_NMS if self._c2v_form == "nms" else nat.C2V_OMS,
                beta=beta, beta_slot=np.arange(g.E, dtype=np.int32),
                alpha=np.ones((rows, 1), np.float32), alpha_slot=np.zeros(g.n, np.int32), **extra)
            self._engine_key, self._uploaded = key, beta
        elif not np.array_equal(beta, self._uploaded):
            self._engine.set_weights(beta, None)
            self._uploaded = beta
        return self._engine

    def forward(self, llr: torch.Tensor, early_stop: bool = True, device=None):
        """-> decoded_bits (int32), posterior (float32), iterations (int / int32[B])"""
        if not isinstance(llr, torch.Tensor):
            raise TypeError("llr must be a torch.Tensor")
        import autograd_bridge as ab
        if ab.wants_grad(self, llr):
            self._refuse_layered_grad("a posterior with a grad_fn")
        _, x, single = _as_batch(llr, self.code.n)
        eng = self._get_engine(x.device if x.is_cuda else device)
        out_dev = llr.device
        if ab.wants_grad(self, llr) and ab.saved_state_fits(eng, x.shape[0]):
            # posterior with a grad_fn back to the edge weights, as in the reference (neural_minsum_decoder.py:100-139)
            g, T = self.code.tanner_graph(), int(self.max_iterations)
            rows, cols = g.check_of_edge.tolist(), g.var_idx.tolist()
            params = [self.beta_weights[f"iter_{t}_c{i}_v{j}"] for t in range(T) for i, j in zip(rows, cols)]
            where = [(t, e) for t in range(T) for e in range(g.E)]
            bt = ab.table_from_params(params, where, (max(T, 1), max(g.E, 1)), 0.0)
            at = torch.ones((max(T, 1), 1), dtype=torch.float32)
            post, bits, iters = ab.decode_train(bt, at, eng, x, bool(early_stop), False)
            if single:
                return bits[0].to(out_dev), post[0].to(out_dev), int(iters[0].item())
            return bits.to(out_dev), post.to(out_dev), iters.to(out_dev)
        if not x.is_cuda and x.shape[0] <= eng.HOST_BATCH_MAX:
            res = eng.decode_host_op(x.detach().to(torch.float32), early_stop=early_stop)
        else:
            res = eng.decode_op(x.detach().to(device=eng.device, dtype=torch.float32), early_stop=early_stop)
        if single:
            return res.bits[0].to(out_dev), res.posterior[0].to(out_dev), int(res.iterations[0].item())
        return res.bits.to(out_dev), res.posterior.to(out_dev), res.iterations.to(out_dev)

    def joint_posterior_loss(self, llr: torch.Tensor, targets: Optional[torch.Tensor] = None,
                             iteration_weights: Optional[torch.Tensor] = None, device=None, *, layered_gradient=None):
        """Posterior joint training with the per-edge weights: the fixed-T decode with
        ``loss = sum_t w_t * mean BCEWithLogits(-posterior_t, targets)`` and its posterior-local gradient, as
        ``Neural2DMinSumDecoder.joint_posterior_loss`` (``layered_gradient`` likewise)
        -> (loss, loss_per_iteration [T], bits, posterior)"""
        import autograd_bridge as ab
        how = ab.check_layered_gradient(self.layered_gradient if layered_gradient is None else layered_gradient, self.schedule)
        if how is None:
            self._refuse_layered_grad("joint_posterior_loss")
        if not isinstance(llr, torch.Tensor):
            raise TypeError("llr must be a torch.Tensor")
        g, T = self.code.tanner_graph(), int(self.max_iterations)
        ab.check_joint_args(self.code.n, T, llr, targets, iteration_weights)
        eng = self._get_engine(llr.device if llr.is_cuda else device)
        rows, cols = g.check_of_edge.tolist(), g.var_idx.tolist()
        params = [self.beta_weights[f"iter_{t}_c{i}_v{j}"] for t in range(T) for i, j in zip(rows, cols)]
        where = [(t, e) for t in range(T) for e in range(g.E)]
        bt = ab.table_from_params(params, where, (max(T, 1), max(g.E, 1)), 0.0)
        at = torch.ones((max(T, 1), 1), dtype=torch.float32)
        return ab.joint_loss(bt, at, eng, llr, targets, iteration_weights, False, layered=how is not None)


class NeuralMinSumDecoder(_EdgeWeightDecoder):
    """Neural MinSum (N-NMS) decoder with edge-specific weights"""

    _c2v_form = "nms"

    def __init__(self, code: LDPCCode, max_iterations: int = 50, *, schedule: str = "flooding", layered_gradient=None):
        import autograd_bridge as ab
        super().__init__()
        self.schedule = check_schedule(schedule)
        self.layered_gradient = ab.check_layered_gradient(layered_gradient, self.schedule)
        self._init_edges(code, max_iterations, offset=0.7)
        num_edges = int(code.tanner_graph().E)
        logger.info(f"Initialized Neural MinSum decoder with {len(self.beta_weights)} parameters")
        logger.info(f"Total edges: {num_edges}, Parameters per iteration: {num_edges}")


class LdpcDecoderNeuralMinSumDecoder(_EdgeWeightDecoder):
    """The SECOND NeuralMinSumDecoder the reference ships, inside ldpc_decoder.py (:155-272): the same per-edge
    normalised min-sum forward, but weights initialised ``randn*0.1`` WITHOUT the +0.7 and an (empty)
    ``alpha_weights`` ParameterDict.  Exported as ``ldpc_decoder.NeuralMinSumDecoder``."""

    def __init__(self, code: LDPCCode, max_iterations: int = 50, *, schedule: str = "flooding", layered_gradient=None):
        import autograd_bridge as ab
        super().__init__()
        self.schedule = check_schedule(schedule)
        self.layered_gradient = ab.check_layered_gradient(layered_gradient, self.schedule)
        self._init_edges(code, max_iterations, offset=0.0)
        self.alpha_weights = nn.ParameterDict()
        logger.info(f"Initialized Neural MinSum decoder with {len(self.beta_weights)} parameters")


LdpcDecoderNeuralMinSumDecoder.__name__ = LdpcDecoderNeuralMinSumDecoder.__qualname__ = "NeuralMinSumDecoder"


class NeuralOffsetMinSumDecoder(_EdgeWeightDecoder):
    """Neural Offset MinSum (N-OMS) decoder with edge-specific offsets"""

    _c2v_form = "oms"

    def __init__(self, code: LDPCCode, max_iterations: int = 50, *, schedule: str = "flooding", layered_gradient=None):
        import autograd_bridge as ab
        super().__init__()
        self.schedule = check_schedule(schedule)
        self.layered_gradient = ab.check_layered_gradient(layered_gradient, self.schedule)
        self._init_edges(code, max_iterations, offset=0.0)
        logger.info(f"Initialized Neural Offset MinSum decoder with {len(self.beta_weights)} parameters")


def analyze_weight_patterns(decoder: _EdgeWeightDecoder, code: LDPCCode) -> Dict:
    """Statistics of the edge weights per iteration and per check-node degree -- same keys and
    numbers as the reference's helper (np.mean/np.std/np.min/np.max over the same weight lists)."""
    g = code.tanner_graph()
    T = int(decoder.max_iterations)
    analysis = {"weight_statistics": {}, "iteration_patterns": {}, "node_degree_correlations": {}}
    if T == 0 or g.E == 0:
        return analysis
    W = decoder.weight_table()[:T, :g.E].astype(np.float64)          # [T, E], values of .item()
    for t in range(T):
        w = W[t]
        analysis["iteration_patterns"][t] = {"mean": np.mean(w), "std": np.std(w), "min": np.min(w), "max": np.max(w)}
    check_degrees = code.check_node_degrees
    dc_of_edge = np.asarray([check_degrees[int(i)] for i in g.check_of_edge])
    edge_mean = np.asarray([np.mean(W[:, e]) for e in range(g.E)])   # average over iterations, per edge
    for dc in set(check_degrees.values()):
        sel = edge_mean[dc_of_edge == dc]
        if sel.size:
            analysis["node_degree_correlations"][f"check_degree_{dc}"] = {
                "mean": np.mean(sel), "std": np.std(sel), "count": int(sel.size)}
    return analysis
