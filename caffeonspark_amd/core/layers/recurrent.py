"""Recurrent layers: LSTM (time-major), Embed.

Caffe's LSTM layer (used by the reference's LRCN captioning net,
data/lrcn_cos.prototxt — SURVEY.md §5 "Long-context") consumes
time-major input x:[T,N,D] plus continuation markers cont:[T,N] and
produces h:[T,N,H].  Upstream implements it by unrolling an internal net;
here it is implemented directly: one big input GEMM over all timesteps,
then a per-step recurrent GEMM + fused LSTM-unit op (the HIP kernel target
for the recurrent path).

By default every forward starts from h = c = 0.  Two opt-ins carry state
across forwards for token-by-token decode: `stateful` (the layer keeps
(h_T, c_T) itself, set through Net.set_recurrent_stateful) and
recurrent_param.expose_hidden (h_0/c_0 bottoms, h_T/c_T tops).  Both run
the per-step loop; a T == 1 step on the bf16 GPU path is one launch of the
fused step kernel (ops/csrc/lstm_step.hip).

Params (upstream-compatible blob order):
  0: W_xc [4H, D]   input-to-gate weights (gate order i,f,o,g)
  1: b_c  [4H]      gate bias
  2: W_hc [4H, H]   hidden-to-gate weights
"""

from __future__ import annotations

import torch

from ... import ops
from ...proto import caffe_pb
from .base import Layer, register_layer


@register_layer("LSTM")
class LSTMLayer(Layer):
    def setup(self, bottom, top):
        p = self.param.recurrent_param
        self.h = int(p.num_output)
        # expose_hidden: bottoms x, cont, [x_static,] h_0, c_0 and tops
        # h, h_T, c_T (recurrent blobs [1, N, H]); stateful: h/c carried
        # from one forward to the next, cont = 0 being the reset
        self.expose = bool(p.expose_hidden)
        self.stateful = bool(getattr(self.net, "recurrent_stateful", False))
        self._state = None
        self.step_route = None
        # "persist" or "loop": which whole-sequence route the last
        # forward / backward of the GPU sequence path took
        self.seq_route = None
        self._wcast = {}
        n_in = len(bottom) - (2 if self.expose else 0)
        if n_in not in (2, 3):
            raise ValueError(
                f"LSTM layer {self.name!r}: {len(bottom)} bottoms with "
                f"expose_hidden={self.expose}; expected x, cont, "
                "[x_static][, h_0, c_0]")
        if self.expose and len(top) != 3:
            raise ValueError(
                f"LSTM layer {self.name!r}: expose_hidden needs the tops "
                "h, h_T, c_T")
        x_shape = bottom[0].shape
        self.t_axis, self.n_axis = 0, 1
        d = 1
        for dim in x_shape[2:]:
            d *= dim
        self.d = d
        self.static = n_in == 3  # x_static bottom
        self.add_param([4 * self.h, d], p.weight_filler, name=self.name + "_Wxc")
        self.add_param([4 * self.h], p.bias_filler, name=self.name + "_bc")
        self.add_param([4 * self.h, self.h], p.weight_filler,
                       name=self.name + "_Whc")
        if self.static:
            self.add_param([4 * self.h, self.d_static(bottom)],
                           p.weight_filler, name=self.name + "_Wxsc")
        self._cache = None

    def d_static(self, bottom):
        ds = 1
        for dim in bottom[2].shape[1:]:
            ds *= dim
        return ds

    # -- carried / exposed hidden state ------------------------------------
    def reset_state(self):
        """Forget the carried (h, c): the next stateful forward starts
        from zeros."""
        self._state = None

    def _step_weight(self, i):
        """Param i in compute dtype without a per-call cast: the solver's
        bf16 shadow where there is one, else a copy cached until the
        master tensor is replaced or written in place."""
        t = self.blobs[i].data
        if t.dtype == self.dtype:
            return t
        sh = getattr(t, "_cos_bf16", None) \
            if self.dtype == torch.bfloat16 else None
        if sh is not None:
            return sh
        hit = self._wcast.get(i)
        if hit is None or hit[0] is not t or hit[1] != t._version:
            hit = (t, t._version, t.to(self.dtype).contiguous())
            self._wcast[i] = hit
        return hit[2]

    def _fused_step_ok(self, tensors, N, Ds):
        """Route of a T == 1 step: the fused kernel serves bf16 on GPU,
        N <= COS_LSTM_STEP_MAXN, 8-aligned segment lengths and a panel
        within its LDS budget; COS_LSTM_STEP=0 turns it off.  It keeps no
        backward cache, so an expose_hidden layer of a TRAIN-phase net
        stays on the per-step ops."""
        x = tensors[0]
        if not x.is_cuda or x.dtype != torch.bfloat16:
            return False
        if not self.stateful and self.phase != caffe_pb.Phase.TEST:
            return False
        return ops.gpu_op("lstm_step_ok")(N, self.d, self.h, Ds, tensors)

    def _forward_step(self, bottom, top):
        """Per-step loop from a given start state: serves expose_hidden
        and stateful layers.  T == 1 on the bf16 GPU path is one fused
        kernel launch (step_route "fused"); everything else is
        ops.fc_forward + ops.lstm_unit_forward per step ("gemm")."""
        if self.expose and self.stateful:
            raise RuntimeError(
                f"LSTM layer {self.name!r}: expose_hidden and stateful are "
                "two ways to carry the state; use one")
        x = bottom[0].data
        cont = bottom[1].data
        T, N = x.shape[0], x.shape[1]
        H = self.h
        if self.expose:
            h_prev = bottom[-2].data.reshape(N, H).to(x.dtype)
            c_prev = bottom[-1].data.reshape(N, H).float()
        else:
            st = self._state
            if st is None or st[0].shape[0] != N \
                    or st[0].device != x.device or st[0].dtype != x.dtype:
                st = (torch.zeros(N, H, dtype=x.dtype, device=x.device),
                      torch.zeros(N, H, dtype=torch.float32,
                                  device=x.device))
            h_prev, c_prev = st
        w_xc, b_c, w_hc = (self._step_weight(0), self._step_weight(1),
                           self._step_weight(2))
        xs = w_xsc = None
        if self.static:
            xs = bottom[2].data.reshape(N, -1)
            w_xsc = self._step_weight(3)
        x2 = x.reshape(T * N, -1)
        if T == 1 and self._fused_step_ok(
                [x2, h_prev, w_xc, w_hc, b_c] +
                ([xs, w_xsc] if self.static else []), N,
                xs.shape[1] if self.static else 0):
            self.step_route = "fused"
            h_t, c_t = ops.gpu_op("lstm_step")(
                x2, h_prev, c_prev, cont[0], w_xc, b_c, w_hc, xs, w_xsc)
            hs = [h_t]
            self._cache = ("fused",)
        else:
            self.step_route = "gemm"
            xg = ops.fc_forward(x2, w_xc, b_c).reshape(T, N, 4 * H)
            if self.static:
                xg = xg + ops.fc_forward(xs, w_xsc, None).unsqueeze(0)
            hs, caches, h_prevs, c_prevs = [], [], [], []
            for t in range(T):
                cont_t = cont[t].reshape(N, 1).to(x.dtype)
                h_in = h_prev * cont_t
                gates = xg[t] + ops.fc_forward(h_in, w_hc, None)
                c_t, h_t, cache = ops.lstm_unit_forward(c_prev, gates,
                                                        cont[t])
                h_prevs.append(h_in)
                c_prevs.append(c_prev)
                caches.append(cache)
                hs.append(h_t)
                c_prev = c_t = c_t.float()
                h_prev = h_t
            self._cache = (x, cont, caches, h_prevs, c_prevs, hs)
        # h_t and c_t are fresh tensors: earlier tops keep their values
        top[0].data = hs[0].reshape(1, N, H) if T == 1 \
            else torch.stack(hs, dim=0)
        if self.expose:
            top[1].data = h_t.reshape(1, N, H)
            top[2].data = c_t.reshape(1, N, H)
        else:
            self._state = (h_t, c_t)
        return 0.0

    def forward(self, bottom, top):
        if self.expose or self.stateful:
            return self._forward_step(bottom, top)
        x = bottom[0].data
        cont = bottom[1].data
        T, N = x.shape[0], x.shape[1]
        H = self.h
        w_xc, b_c, w_hc = (self.weight(0), self.weight(1), self.weight(2))
        xg = ops.fc_forward(x.reshape(T * N, -1), w_xc, b_c).reshape(T, N, 4 * H)
        if self.static:
            xs = ops.fc_forward(bottom[2].data.reshape(N, -1), self.weight(3),
                                None)
            xg = xg + xs.unsqueeze(0)
        seq_fwd = ops.gpu_op("lstm_seq_forward") if x.is_cuda else None
        if seq_fwd is not None:
            # whole recurrence driven from C++ (3 kernel launches/step)
            ctx = {}
            y, seq_cache = seq_fwd(xg, w_hc, cont, ctx)
            self.seq_route = ctx["route"]
            top[0].data = y
            self._cache = ("seq", x, cont, seq_cache)
            return 0.0
        h_prev = torch.zeros(N, H, dtype=x.dtype, device=x.device)
        c_prev = torch.zeros(N, H, dtype=torch.float32, device=x.device)
        hs, caches, h_prevs, c_prevs = [], [], [], []
        for t in range(T):
            cont_t = cont[t].reshape(N, 1).to(x.dtype)
            h_in = h_prev * cont_t
            gates = xg[t] + ops.fc_forward(h_in, w_hc, None)
            c_t, h_t, cache = ops.lstm_unit_forward(c_prev, gates, cont[t])
            h_prevs.append(h_in)
            c_prevs.append(c_prev)
            caches.append(cache)
            hs.append(h_t)
            c_prev = c_t.float()
            h_prev = h_t
        y = torch.stack(hs, dim=0)
        top[0].data = y
        self._cache = (x, cont, caches, h_prevs, c_prevs, hs)
        return 0.0

    def backward(self, top, propagate_down, bottom):
        if self.stateful:
            raise RuntimeError(
                f"LSTM layer {self.name!r} is stateful (decode only): "
                "training through carried state is not supported")
        if self._cache and isinstance(self._cache[0], str) \
                and self._cache[0] == "seq":
            self._backward_seq(top, propagate_down, bottom)
            return
        if self._cache and isinstance(self._cache[0], str) \
                and self._cache[0] == "fused":
            raise RuntimeError(
                f"LSTM layer {self.name!r}: the fused decode step keeps no "
                "backward cache; set COS_LSTM_STEP=0 to differentiate a "
                "T == 1 expose_hidden step")
        x, cont, caches, h_prevs, c_prevs, hs = self._cache
        T, N = x.shape[0], x.shape[1]
        H = self.h
        w_xc, w_hc = self.weight(0), self.weight(2)
        dy = top[0].diff
        d_xg = torch.zeros(T, N, 4 * H, dtype=torch.float32, device=x.device)
        dw_hc = torch.zeros_like(self.blobs[2].data)
        dh_next = torch.zeros(N, H, dtype=torch.float32, device=x.device)
        dc_next = torch.zeros(N, H, dtype=torch.float32, device=x.device)
        if self.expose:
            # h_T / c_T are tops of their own: their diffs seed the
            # recurrent gradients
            if top[1].diff is not None:
                dh_next = top[1].diff.reshape(N, H).float()
            if top[2].diff is not None:
                dc_next = top[2].diff.reshape(N, H).float()
        for t in reversed(range(T)):
            dh = (dy[t].float() if dy is not None else 0) + dh_next
            dc_prev, d_gates = ops.lstm_unit_backward(
                c_prevs[t], caches[t], dc_next, dh.to(x.dtype))
            d_gates_f = d_gates.float()
            d_xg[t] = d_gates_f
            # gates_t = xg[t] + h_in @ w_hc^T ; h_in = h_{t-1} * cont_t
            dh_in = d_gates_f @ w_hc.float()
            dw_hc += d_gates_f.t() @ h_prevs[t].float()
            cont_t = cont[t].reshape(N, 1).float()
            dh_next = dh_in * cont_t
            dc_next = dc_prev
        if self.expose:
            # after t = 0 the carried gradients are those of h_0 / c_0
            ih, ic = len(bottom) - 2, len(bottom) - 1
            if propagate_down[ih]:
                b = bottom[ih]
                self.acc_blob_diff(
                    b, dh_next.reshape(b.data.shape).to(b.data.dtype), False)
            if propagate_down[ic]:
                b = bottom[ic]
                self.acc_blob_diff(
                    b, dc_next.reshape(b.data.shape).to(b.data.dtype), False)
        # input GEMM backward
        d_xg_flat = d_xg.reshape(T * N, 4 * H)
        if propagate_down[0]:
            dx = (d_xg_flat @ w_xc.float()).reshape(x.shape)
            self.acc_blob_diff(bottom[0], dx.to(x.dtype), False)
        if self.blobs[0]._lr_mult != 0:
            self.acc_param_diff(0, d_xg_flat.t() @ x.reshape(T * N, -1).float())
            self.acc_param_diff(1, d_xg_flat.sum(0))
            self.acc_param_diff(2, dw_hc)
        if self.static and self.blobs[3]._lr_mult != 0:
            xs = bottom[2].data.reshape(N, -1).float()
            d_static = d_xg.sum(dim=0)  # [N, 4H]
            self.acc_param_diff(3, d_static.t() @ xs)
            if propagate_down[2]:
                dxs = d_static @ self.weight(3).float()
                self.acc_blob_diff(bottom[2],
                                   dxs.reshape(bottom[2].data.shape).to(x.dtype),
                                   False)


    def _backward_seq(self, top, propagate_down, bottom):
        _, x, cont, seq_cache = self._cache
        T, N = x.shape[0], x.shape[1]
        H = self.h
        dy = top[0].diff
        seq_bwd = ops.gpu_op("lstm_seq_backward")
        ctx = {}
        dxg, dw_hc = seq_bwd(dy.reshape(T, N, H), self.weight(2), seq_cache,
                             ctx)
        self.seq_route = ctx["route"]
        dxg_flat = dxg.reshape(T * N, 4 * H)
        x_flat = x.reshape(T * N, -1)
        # shared tail: input GEMM grads == a linear layer's backward
        dx, dw_xc, db = ops.fc_backward(
            x_flat, self.weight(0), dxg_flat,
            need_dx=propagate_down[0], bias=True)
        if self.blobs[0]._lr_mult != 0:
            self.acc_param_diff(0, dw_xc)
            self.acc_param_diff(1, db)
            self.acc_param_diff(2, dw_hc)
        if propagate_down[0]:
            self.acc_blob_diff(bottom[0], dx.reshape(x.shape), False)
        if self.static and self.blobs[3]._lr_mult != 0:
            xs = bottom[2].data.reshape(N, -1)
            d_static = dxg.float().sum(dim=0)  # [N, 4H]
            self.acc_param_diff(3, d_static.t() @ xs.float())
            if propagate_down[2]:
                dxs = (d_static @ self.weight(3).float()).to(x.dtype)
                self.acc_blob_diff(bottom[2],
                                   dxs.reshape(bottom[2].data.shape), False)


@register_layer("Embed")
class EmbedLayer(Layer):
    def setup(self, bottom, top):
        p = self.param.embed_param
        self.e = int(p.num_output)
        self.v = int(p.input_dim)
        self.bias_term = p.bias_term
        self.add_param([self.v, self.e], p.weight_filler, name=self.name + "_w")
        if self.bias_term:
            self.add_param([self.e], p.bias_filler, name=self.name + "_b")

    def forward(self, bottom, top):
        idx = bottom[0].data
        w = self.weight(0)
        b = self.cast(self.blobs[1].data) if self.bias_term else None
        y = ops.embed_forward(idx.reshape(idx.shape[0], -1) if idx.dim() > 2
                              else idx, w, b)
        # caffe embed output: bottom shape (with trailing singleton dims
        # dropped) + [E]
        base = [s for s in idx.shape]
        # drop trailing singleton SPATIAL dims but never the batch axis
        # (time-major [T, 1] single-image decode must stay 2-d)
        while len(base) > 2 and base[-1] == 1:
            base = base[:-1]
        top[0].data = y.reshape(base + [self.e])
        return 0.0

    def backward(self, top, propagate_down, bottom):
        if propagate_down[0]:
            raise RuntimeError("Embed cannot backprop to indices")
        if self.blobs[0]._lr_mult == 0:
            return
        idx = bottom[0].data
        dy = top[0].diff.reshape(-1, self.e)
        dw, db = ops.embed_backward(idx, dy, self.v, self.bias_term)
        self.acc_param_diff(0, dw)
        if db is not None:
            self.acc_param_diff(1, db)
