"""float64 reference and error bounds of the sequence loss (csrc/seqloss.hip: mvlt_seq_loss_plan, mvlt_seq_loss_fwd,
mvlt_ce_bwd_weighted), in the manner of misc_ref.py / head_ce_ref.py: references are taken from the SAME operands the kernels read
(bf16 and f32 values are exact in float64), U = U32 = 2^-24 is one f32 rounding, u_out(dtype) the rounding of the stored type, and
every reported bound is SAFETY times the first-order estimate plus a tiny absolute term.

The plan (plan_ref) is integers and copies: plain Python over rows, compared with torch.equal.

    len_b = 1 + index of the first eos, else the index of the first id <= 0, else T            N = sum_b len_b
    slot off_b + t  <-  position (b, t), t < len_b: row row0 + b row_step + t, label ids[b, t], weight w[b, t]
    slot N + k      <-  the k-th position behind an end, in (b, t) order: its row, label -100, weight 0
    tf_ids          =   ids on the scored positions, 0 behind them; a negative id ahead of an eos: label -100, weight 0, tf id 0
                        (it keeps its slot inside the prefix and counts in N: the one case where the packing is not the stable
                        partition ops.label_plan makes of the implied labels)

The weighted sum (mvlt_seq_loss_fwd) over the n = *rows_dev packed rows, term_i = w_i (lse_i - x_i), rows of weight 0 left out:
  the subtraction and the product round once each: 2 U |term_i|;  thread t adds its ceil(n / 1024) terms in order and a binary
  tree of depth 10 adds the 1024 partial sums, so a term passes through at most ceil(n / 1024) - 1 + 10 additions, each of
  which rounds a partial sum no larger than sum |term| (order known, worst case over magnitudes, no sqrt(n)):
                                                   e_sum = (ceil(n / 1024) + 9 + 2) U sum_i |term_i|

The weighted backward (mvlt_ce_bwd_weighted) takes lse, count and the weights as exact (f32 values it is handed):
  c_i = fl(fl(fl(gscale gscale_dev) / max(count, 1)) w_i): three roundings, 3 U relative.
  dl = c_i (exp(x - lse) - [n == label]):  t = x - lse rounds once (U |t| on t), __expf(t) = exp2(t log2 e) rounds the product
  (another U |t| relative) and the hardware exp2 is good to 1 ulp = 2 U, one spare: (2 |t| + 3) U p as in misc_ref; the
  subtraction and the product with c_i round once each, then the store:
                                                   e_dl = |c_i| (2 |t| + 3) U p + (5 U + U_OUT) |dl|
  Rows with a negative label or weight 0, the columns V .. ld - 1: exactly 0.  -inf logits give p = 0 on both sides."""
import math

import torch

from attn_ref import SAFETY, U32, U_BF16  # noqa: F401
from gemm_ref import check_bound  # noqa: F401  (re-exported)
from ln_ref import check_untouched, u_out  # noqa: F401
from misc_ref import TINY, check_equal, check_zero, f32, gen  # noqa: F401

BF, F32 = torch.bfloat16, torch.float32
IGNORE = -100


# ------------------------------------------------------------------ plan
def seq_len(row, eos):
    """len of one id row (a list of ints)."""
    if eos is not None and eos >= 0 and eos in row:
        return row.index(eos) + 1
    for t, v in enumerate(row):
        if v <= 0:
            return t
    return len(row)


def plan_ref(ids, eos, weights, row0, row_step):
    """ids: int64 [B, T] tensor; weights f32 [B] or [B, T].  -> dict of tensors: len i32 [B], tf_ids i64 [B, T], gather_row i32
    [B T], sel_labels i64 [B T], row_weight f32 [B T], rows (int N)."""
    B, T = ids.shape
    rows = ids.tolist()
    w = weights.tolist()
    lens = [seq_len(r, eos) for r in rows]
    N = sum(lens)
    gather, labels, rw = [0] * (B * T), [IGNORE] * (B * T), [0.0] * (B * T)
    tf = [[0] * T for _ in range(B)]
    head, tail = 0, N
    for b in range(B):
        for t in range(T):
            row = row0 + b * row_step + t
            if t < lens[b]:
                v = rows[b][t]
                gather[head] = row
                if v >= 0:
                    labels[head], tf[b][t] = v, v
                    rw[head] = w[b][t] if weights.dim() == 2 else w[b]
                head += 1
            else:
                gather[tail] = row
                tail += 1
    assert head == N and tail == B * T
    return dict(len=torch.tensor(lens, dtype=torch.int32), tf_ids=torch.tensor(tf, dtype=torch.int64).reshape(B, T),
                gather_row=torch.tensor(gather, dtype=torch.int32), sel_labels=torch.tensor(labels, dtype=torch.int64),
                row_weight=torch.tensor(rw, dtype=torch.float32), rows=N)


def implied_labels(ids, eos):
    """int64 [B, T]: ids on the scored positions (a negative id there: -100), -100 behind the ends -- the labels whose
    ops.label_plan is the plan's gather_row / sel_labels / rows_dev."""
    B, T = ids.shape
    out = torch.full((B, T), IGNORE, dtype=torch.int64)
    for b, r in enumerate(ids.tolist()):
        n = seq_len(r, eos)
        out[b, :n] = torch.tensor([v if v >= 0 else IGNORE for v in r[:n]], dtype=torch.int64)
    return out


EOS = 104


def plan_ids(B, T, seed):
    """Rows with the edges in turn: eos at 0 / the middle / T - 1, no eos and no PAD, a PAD ahead of an eos, all PAD, a PAD and no
    eos; the rest random lengths.  Ids are 1 .. 2999 with no accidental EOS.  (No negative ids: with one ahead of an eos the plan
    keeps a slot label_plan would move, see the module text.)"""
    g = gen(seed)
    ids = torch.randint(1, 3000, (B, T), generator=g)
    ids[ids == EOS] = EOS + 1
    for b in range(B):
        kind = b % 8
        if kind == 0:
            ids[b, 0] = EOS
        elif kind == 1:
            ids[b, T // 2] = EOS
            ids[b, T // 2 + 1:] = 0
        elif kind == 2:
            ids[b, T - 1] = EOS
        elif kind == 3:
            pass                                         # runs to T
        elif kind == 4:
            ids[b, T // 3] = 0                           # PAD ahead of an eos: the eos still ends the row
            ids[b, min(T - 1, T // 3 + 2)] = EOS
        elif kind == 5:
            ids[b] = 0
        elif kind == 6:
            ids[b, (2 * T) // 3:] = 0                    # PAD-terminated, no eos
        else:
            n = int(torch.randint(0, T + 1, (1,), generator=g))
            ids[b, n:] = 0
            if n:
                ids[b, n - 1] = EOS
    return ids


def plan_weights(B, T, layout, seed):
    g = gen(seed)
    w = torch.randn(B, T if layout == "bt" else 1, generator=g)
    w[0] = 0.0
    return w if layout == "bt" else w[:, 0].contiguous()


# ------------------------------------------------------------------ weighted sum
def seq_sum_ref(lse, x_label, row_weight, n):
    """(sum, bound, n) over the first n rows; rows of weight 0 add nothing whatever their lse / x_label hold."""
    w = row_weight[:n].double()
    d = lse[:n].double() - x_label[:n].double()
    term = torch.where(w != 0, w * torch.where(w != 0, d, torch.zeros_like(d)), torch.zeros_like(d))
    adds = math.ceil(max(n, 1) / 1024) - 1 + 10
    return float(term.sum()), SAFETY * (adds + 2) * U32 * float(term.abs().sum()) + TINY, n


# ------------------------------------------------------------------ weighted backward
def coeff(gscale, gscale_dev, count, row_weight):
    """c_i in float64 from the f32 values the kernel is handed."""
    sc = f32(gscale) * (1.0 if gscale_dev is None else f32(gscale_dev)) / max(float(count), 1.0)
    return sc * row_weight.double()


def weighted_dl_ref(x, V, labels, lse, row_weight, count, gscale, gscale_dev, dtype, n_valid=None, c=None):
    """-> (dl, bound) [n_valid, V] float64; ignored and zero-weight rows are 0.  ``c`` replaces the coefficients (the CPU test's
    wrong results)."""
    n_valid = x.shape[0] if n_valid is None else n_valid
    xv, lab = x[:n_valid, :V].double(), labels[:n_valid]
    c = coeff(gscale, gscale_dev, count, row_weight[:n_valid]) if c is None else c[:n_valid]
    live = ((lab >= 0) & (c != 0))[:, None]
    t = xv - lse[:n_valid].double()[:, None]
    t = torch.where(live, t, torch.zeros_like(t))
    p = torch.exp(t)
    hot = torch.arange(V)[None, :] == lab[:, None]
    dl = torch.where(live, c[:, None] * (p - hot.double()), torch.zeros_like(p))
    fin = torch.where(torch.isfinite(t), t.abs(), torch.zeros_like(t))
    b = c.abs()[:, None] * (2.0 * fin + 3.0) * U32 * p + (5.0 * U32 + u_out(dtype)) * dl.abs()
    return dl, torch.where(live, SAFETY * b, torch.zeros_like(b)) + TINY


def ceil64(v):
    return (v + 63) // 64 * 64


GSCALE, GSCALE_DEV = 0.5, 3.0
# (rows, V, ld): ld = ceil64(V) -- the head's layout --, and one ld that is no multiple of 4 (the element-wise route)
SHAPES = ((5, 67, 128), (9, 3000, 3008), (4, 30522, 30528), (5, 67, 70))
SMALL = SHAPES[:2] + SHAPES[3:]                              # the CPU test's table
ZERO_ROW, IGNORED_ROW = 3, 2


def weighted_case(rows, V, ld, dtype, seed, n_valid=None):
    """Operands of one backward case: x [rows, ld] in ``dtype`` (columns V .. and rows n_valid .. NaN), labels (row 0: column
    V - 1, row 1: column 0, row 2: ignored), the zero-weight row 3 holding a +inf logit, lse f32 of the stored logits, count.
    Weights: 1e3, -0.75, (2 on the ignored row), 0, 1, then 2, -1.5, 1, 0.25 in turn -- 0, a negative one, 1 and 1e3 all on
    LIVE rows, neighbours different wherever both rows are live.  The 4-row shape has three live rows for those four values:
    there rows 0 and 1 carry -1e3 and 1 (the negative weight and the magnitude 1e3 on one row)."""
    assert rows >= 4
    g = gen(seed)
    x = 3.0 * torch.randn(rows, V, generator=g)
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[0], labels[1], labels[IGNORED_ROW] = V - 1, 0, IGNORE
    x[ZERO_ROW, V // 2] = math.inf
    head = [-1e3, 1.0, 2.0, 0.0] if rows == 4 else [1e3, -0.75, 2.0, 0.0, 1.0]
    w = torch.tensor((head + [2.0, -1.5, 1.0, 0.25] * rows)[:rows], dtype=torch.float32)
    assert w[IGNORED_ROW] != 1.0 and labels[ZERO_ROW] >= 0 and any(w[r] == 1.0 and labels[r] >= 0 for r in range(rows))
    full = torch.full((rows, ld), math.nan)
    full[:, :V] = x
    if n_valid is not None:
        full[n_valid:] = math.nan
    xs = full.to(dtype)
    lse = torch.logsumexp(xs[:, :V].double(), 1).float()
    count = float((labels[:rows if n_valid is None else n_valid] >= 0).sum())
    return xs, labels, w, lse, count
