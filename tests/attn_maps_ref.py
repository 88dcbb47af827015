"""float64 reference of an mvlt_attn_probs call and its per-element bound, built on tests/attn_ref.py.

The probabilities are recomputed from a GIVEN lse, P = exp(s - lse_given), with s the float64 logits of AttnRef (the masks
come from the oracle's statements through bert_bias, keys a packed sequence does not have are MASK_OUT).  The bound is the one
attn_ref.py uses for "P recomputed from the saved lse" (relPb):

    |dP| <= SAFETY P (ds + lse_err + C_EXP U32 + 2 U32 |s - lse| + U32) + 1e-30,
    ds = C_ACC U32 sqrt(hd) scale |q|.|k| + 2 U32 |s|          (the f32 logit, as in AttnRef)

lse_err is U32 |lse| when the test feeds the float64 lse rounded to f32, and AttnRef.lse_b when the lse comes from
mvlt_attn_fwd.  Query rows a packed sequence does not have are rows of zeros.  Entries the reference has at exactly 0 carry the
1e-30 only; check_maps asserts they are exactly 0 as well.

HEAD_MEAN: the mean of the per-head references; the bound is the mean of the per-head bounds plus nH U32 mean (the nH f32
additions and the division).  RENORM: R = P / S with S the row sum over the selected keys; to first order
dR = (dP + R sum(dP)) / S, plus 2 U32 R for the f32 row sum's last roundings and the division (the sum's own error,
C_ACC U32 sqrt(nk) S, enters as R C_ACC U32 sqrt(nk)).  A row whose sum is 0 stays 0.  With both flags the mean comes first:
the row that is renormalised is the OUTPUT row."""
import math

import torch

from attn_ref import C_ACC, C_EXP, SAFETY, U32, _heads, check_bound


class MapsRef:
    """P = exp(s - lse_given) and its bound for every (sequence, head, query, key), from an AttnRef of the same operands.
    qkv: the kernel's operand; ref: AttnRef(qkv, None, ...) ; lse_given [nseq, nH, L]: the values the kernel reads (f32);
    lse_err [nseq, nH, L]: the bound on their error against the float64 lse.  select() cuts a call's output out of it."""

    def __init__(self, ref, qkv, lse_given, lse_err, *, nseq, L, nH, hd, scale, pack=None):
        dev = ref.s.device
        C = nH * hd
        row_index = None if pack is None else pack[0].to(dev)
        Q = _heads(qkv[:, :C].to(dev), nseq, L, nH, hd, row_index)
        K = _heads(qkv[:, C:2 * C].to(dev), nseq, L, nH, hd, row_index)
        s = ref.s
        qvalid = torch.isfinite(ref.lse)                                # [nseq, nH, L]: queries the sequence has
        lse = torch.where(qvalid, lse_given.double().to(dev), torch.zeros_like(ref.lse))[..., None]
        err = torch.where(qvalid, lse_err.double().to(dev), torch.zeros_like(ref.lse))[..., None]
        P = torch.exp(s - lse) * qvalid[..., None]
        ds = C_ACC * U32 * math.sqrt(hd) * scale * (Q.abs() @ K.abs().transpose(-1, -2)) + 2 * U32 * s.abs()
        rel = ds + err + C_EXP * U32 + 2 * U32 * (s - lse).abs() + U32
        self.P = P
        self.dP = torch.where(P > 0, P * rel, torch.zeros_like(P))     # (0 * a huge |s| of a masked key stays 0)
        self.nH = nH

    def select(self, q_range, k_range, head_mean=False, renorm=False):
        """(want, bound) f64 [nseq, nH or 1, nq, nk] of a call with these ranges and flags."""
        (q0, nq), (k0, nk) = q_range, k_range
        P = self.P[:, :, q0:q0 + nq, k0:k0 + nk]
        dP = self.dP[:, :, q0:q0 + nq, k0:k0 + nk]
        if head_mean:
            P = P.mean(1, keepdim=True)
            dP = dP.mean(1, keepdim=True) + self.nH * U32 * P
        if renorm:
            S = P.sum(-1, keepdim=True)
            ok = S > 0
            Ss = torch.where(ok, S, torch.ones_like(S))
            R = torch.where(ok, P / Ss, torch.zeros_like(P))
            dP = torch.where(ok, (dP + R * dP.sum(-1, keepdim=True)) / Ss + (2 * U32 + C_ACC * U32 * math.sqrt(nk)) * R,
                             torch.zeros_like(P))
            P = R
        return P, SAFETY * dP + 1e-30


def maps_case(s2s, dtype, seed, *, n_img=49, T=23, lens=(23, 9, 1), image_mask_zeros=True, packed=False, nH=2, hd=64):
    """One MVLBert attention layout on the host: sequences with caption lengths `lens` (ids zero-padded to T), optionally an
    image_mask with zeros on sequence 1, dense rows or packed rows (pack_layout with gaps of NaN rows, each sequence cut
    after its caption).  Returns a dict: qkv, ids, im, bias (oracle statements), ref (AttnRef, forward only), kw (the AttnRef
    geometry), pack = (row_start, seq_len, rows, row_index) or None, n_img, T, L."""
    from attn_ref import AttnRef, attn_operands, bert_bias, pack_layout
    nseq, L = len(lens), n_img + 2 + T
    ids = torch.zeros(nseq, T, dtype=torch.long)
    for b, ln in enumerate(lens):
        ids[b, :ln] = 5 + torch.arange(ln)
    im = None
    if image_mask_zeros and not s2s:
        im = torch.ones(nseq, n_img, dtype=torch.uint8)
        im[1 % nseq, 0] = im[1 % nseq, n_img // 2] = im[1 % nseq, -1] = 0
    pack = None
    rows = row_index = None
    if packed:
        row_start, seq_len, rows, row_index = pack_layout([n_img + 2 + ln for ln in lens], L, gap=3)
        pack = (row_start, seq_len, rows, row_index)
    qkv, _ = attn_operands(nseq, L, nH, hd, dtype, seed, rows=rows, row_index=row_index)
    bias = bert_bias(s2s, nseq, L, n_img, ids, im)
    kw = dict(nseq=nseq, L=L, nH=nH, hd=hd, scale=hd ** -0.5)
    ref = AttnRef(qkv, None, bias=bias, dtype=dtype, pack=None if pack is None else (row_index, seq_len), **kw)
    return dict(qkv=qkv, ids=ids, im=im, bias=bias, ref=ref, kw=kw, pack=pack, n_img=n_img, T=T, L=L, s2s=s2s, dtype=dtype)


FLAGS = [(False, False), (True, False), (False, True), (True, True)]          # (head_mean, renorm)


def recording_dropper():
    """An eval-mode oracle Dropper that keeps what the attention dropout of every layer is handed -- the softmax probabilities
    -- under its tag ('<layer prefix>.attn_drop').  oracle/ itself is not edited: a subclass."""
    from oracle import mvlt_oracle as O

    class Recorder(O.Dropper):
        def __init__(self):
            super().__init__("off")
            self.probs = {}

        def __call__(self, x, p, tag):
            if tag.endswith(".attn_drop"):
                self.probs[tag] = x
            return x
    return Recorder()


def check_maps(out, want, bound, what):
    """Every element within its bound, and exactly 0 where the reference is exactly 0.  out / want / bound: [nseq, H, nq, nk]."""
    assert tuple(out.shape) == tuple(want.shape), (what, tuple(out.shape), tuple(want.shape))
    o = out.detach().double().cpu().reshape(-1, out.shape[-1])
    w, b = want.cpu().reshape(-1, want.shape[-1]), bound.cpu().reshape(-1, want.shape[-1])
    check_bound(o, w, b, f"{what} (row = ((sequence * heads) + head) * nq + query, column = key)")
    zero = w == 0
    assert bool((o[zero] == 0).all()), f"{what}: {int((o[zero] != 0).sum())} entries the reference has at exactly 0 are not 0"


def worst_ratio(out, want, bound):
    return float(((out.detach().double().cpu() - want.cpu()).abs() / bound.cpu()).max())
