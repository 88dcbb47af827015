"""float64 references and per-element error bounds for the training-step kernels of csrc/misc.hip: cross entropy, AdamW,
the VL embeddings, column sums, the row movers and the elementwise kernels.

Every reference is taken from the SAME operands the kernel reads (bf16 and f32 values are exact in float64) and the
hyperparameters are the f32 values the C ABI carries.  U = U32 = 2^-24 is one f32 rounding, U_OUT the rounding of the output
type (u_out), C_ACC sqrt(n) the project's constant for an f32 sum of n terms.  Every reported bound is SAFETY times the
first-order estimate plus a tiny absolute term, except colsum_ref, which keeps the form of gemm_ref.colsum_ref.
tests/test_misc_bound_cpu.py proves on the host that an f32 emulation of each kernel stays inside these bounds and that
local damage is rejected with its place named; tests/test_misc_routes_gpu.py runs the kernels against them.

Cross entropy (ce_fwd_kernel / ce_bwd_kernel), one row of V logits x, label lab, mx = max_c x (exact):
  t_c = x_c - mx, one rounding for f32 logits (two bf16 values far apart do not subtract exactly either): U |t| on t.
  __expf(t) = exp2(t log2 e): the rounded product moves the exponent by U |t| log2 e, a relative U |t| on the result; the
  hardware exp2 is good to 1 ulp = 2 U; one spare:  e_c = (2 |t_c| + 3) U exp(t_c).  Terms below 2^-126 flush to 0, an
  absolute 1.2e-38 per term against s >= 1.
  s = sum_c exp(t_c) >= 1 in f32 (per-lane partial sums at stride 1024, wave butterflies, four waves):
                                                   e_s = sum_c e_c + C_ACC U sqrt(V) s
  lse = mx + logf(s): logf is good to 1 ulp of its result, the addition rounds once:
                                                   e_lse = e_s / s + 2 U |log s| + U |lse|
  loss_sum = sum over the n labelled rows of term_r = lse_r - x[r, lab] (one subtraction each: U |term_r|), added by f32
  atomics in ARBITRARY order, so the order-free worst case and no sqrt(n):
                                                   e_loss = (n - 1) U sum_r |term_r| + sum_r (e_lse_r + U |term_r|)
  count is exact (f32 counts integers below 2^24 exactly).
  The backward takes the lse and the count it is handed as exact (the forward is where they are judged).
  sc = gscale gscale_dev / max(count, 1): two roundings.  dl_c = sc (exp(x_c - lse) - [c == lab]): the exponential as
  above (p = exp(x - lse)), the subtraction and the product round once each:
                                                   e_dl = |sc| (2 |x - lse| + 3) U p + 4 U |dl| + U_OUT |dl|
  (a first estimate of (|x - lse| + 3) U p + 3 U |dl| leaves out the rounding of the subtraction x - lse and the second
  rounding of sc: the f32 emulation of test_misc_bound_cpu.py reaches 1.6 times that estimate, 0.79 of its bound, and 0.43
  of this one.  In e_lse the same 2 |t| and the logf term are dominated by C_ACC sqrt(V): the emulation's worst ratio is
  0.31 with or without them.)  -inf logits give p = 0 exactly on both sides and carry no error term.

AdamW (adamw_sweep), torch's single-tensor formula with f32 hyperparameters, bc1 = (float)(1 - pow((double)b1, step)),
bc2s = (float)sqrt(1 - pow((double)b2, step)), gr = g gs (gs = gscale, or the f32 product gscale coef of the guarded form):
  m' = b1 m + (1 - b1) gr         1 - b1 is exact (Sterbenz); gr, the two products and the sum round:
                                                   e_m = U (|b1 m| + 2 |(1 - b1) gr| + |m'|)
  v' = b2 v + (1 - b2) gr gr      gr enters twice, three products and the sum, and results below 2^-126 are denormal:
                                                   e_v = U (|b2 v| + 4 (1 - b2) gr^2 + v') + V_FLOOR,  V_FLOOR = 2^-125
         (the floor covers a flush to zero of the product and of the sum as well as the coarser denormal grid, so the
         check passes on either behaviour; test_misc_routes_gpu.py records which one the device shows: the MI355X keeps
         f32 denormals in exp_avg_sq, it does not flush them)
  p1 = p (1 - lr wd)              two roundings in the factor, one in the product:   e_p1 = 3 U |p1|
  r  = sqrtf(v') (correctly rounded).  d sqrt / d v is unbounded at v -> 0, but |sqrt(a) - sqrt(b)| <= sqrt|a - b| always:
                                                   e_r = min(e_v / (2 sqrt v'), sqrt e_v) + U r
  den = r / bc2s + eps            e_den = e_r / bc2s + U r / bc2s + U den
  q  = (lr / bc1) m' / den        e_q = (lr / bc1) (e_m / den + |m'| e_den / den^2) + 3 U |q|
  p' = p1 - q                     e_p = e_p1 + e_q + U |p'|
  The bf16 shadow is the rounding of the stored p', asserted with torch.equal.

Embeddings.  The forward is (src + type) + pos in f32 in that order, rounded to the output type: embed_statement states it
with torch's own IEEE f32 additions and the kernel must equal it bit for bit.  The backward: dimage is a copy; dword is a
scatter-add by f32 atomics onto what the caller left (k hits onto a prior value are k + 1 summands in arbitrary order):
                                                   e_dword = k U (|prior| + sum |g|)
  (the [CLS] / [SEP] rows receive prior + an ordered batch sum, which the same expression covers); a row hit once must
  equal the f32 sum prior + g exactly, an untouched row keeps its bits.  dpos and dtype_emb are overwritten with ordered
  f32 sums of n terms (n = B for a position row, B times the positions of a type for a type row):
                                                   e_sum = C_ACC U sqrt(n) sum |term| + U |sum|
  and every row that receives no gradient is exactly 0.

Column sums (colsum_partial_kernel / colsum_final_kernel): gemm_ref.colsum_ref's form, C_ACC U sqrt(M) sum_m |x|, plus
U |result| for the addition onto the previous content under accumulate.

Elementwise (unary_kernel), with g = gelu(x), d = dy gelu'(x) as in gemm_ref / ln_ref:
  gelu      ERFC_ABS |x| + 4 U |g| + U_OUT |g|            gelu_bwd  ERFC_ABS |dy| + 4 U |d| + U_OUT |d|
  tanh      4 U |y| + U_OUT |y|   (tanhf: 2 ulp)           tanh_bwd  U |dy| (y^2 + 2 |1 - y^2|) + U_OUT |dx|
The movers (rows_transform without dropout, rows_scatter, im2col, cast) have plain statements and are compared with
torch.equal."""
import math

import torch

from attn_ref import C_ACC, SAFETY, U32, U_BF16, keep_ref  # noqa: F401  (keep_ref re-exported)
from gemm_ref import ERFC_ABS, check_bound, gelu64, gelu_grad64  # noqa: F401  (check_bound re-exported)
from ln_ref import check_untouched, u_out  # noqa: F401

BF, F32 = torch.bfloat16, torch.float32
IGNORE = -100
V_FLOOR = 2.0 ** -125
TINY = 1e-30


def f32(v):
    """The f32 value the C ABI carries for a Python float."""
    return float(torch.tensor(v, dtype=torch.float32))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def check_equal(out, ref, what):
    """Bit-level equality of values (NaN equals NaN, -0.0 differs from 0.0); a failure names the first element that differs."""
    assert out.shape == ref.shape and out.dtype == ref.dtype, (what, tuple(out.shape), tuple(ref.shape), out.dtype, ref.dtype)
    if out.numel() == 0:
        return
    a = out.reshape(out.shape[0], -1) if out.dim() > 1 else out.reshape(-1, 1)
    b = ref.to(out.device).reshape(a.shape)
    same = ((a == b) & (torch.signbit(a) == torch.signbit(b))) | (torch.isnan(a) & torch.isnan(b))
    if not bool(same.all()):
        bad = (~same).nonzero()[0]
        r, c = int(bad[0]), int(bad[1])
        raise AssertionError(f"{what}: {int((~same).sum())} of {a.numel()} elements differ; first at row {r}, column {c}: "
                             f"out {float(a[r, c])!r}, expected {float(b[r, c])!r}")


def check_zero(out, what):
    """Every element is exactly 0 (either sign); a failure names the first one that is not."""
    if out.numel() == 0:
        return
    a = out.reshape(out.shape[0], -1) if out.dim() > 1 else out.reshape(-1, 1)
    if not bool((a == 0).all()):
        bad = (a != 0).nonzero()[0]
        r, c = int(bad[0]), int(bad[1])
        raise AssertionError(f"{what}: {int((a != 0).sum())} of {a.numel()} elements are not 0; first at row {r}, column {c}: "
                             f"{float(a[r, c])!r}")


# ------------------------------------------------------------------ cross entropy
CE_SHAPES = ((2, 4), (3, 3), (1023, 1023), (1024, 1024), (1025, 1028), (1027, 1027), (3000, 3008), (30522, 30528),
             (30522, 30522))
CE_FAMILIES = ("plain", "confident", "wide", "flat", "masked")
CE_ROWS = {"third-ignored": (37, None), "one-row": (1, None), "ragged": (40, 23)}      # name -> (rows, *rows_dev)
CE_GSCALE, CE_GSCALE_DEV = 0.5, 3.0


def ce_labels(rows, V, seed, ignore="third"):
    """Row 0: the last valid column; row 1: the first column of the last 4-column group (the group that straddles V when
    V % 4 != 0).  ignore: "third" (rows 2, 5, 8, ...), "all" or "none"."""
    lab = torch.randint(0, V, (rows,), generator=gen(seed))
    lab[0] = V - 1
    if rows > 1:
        lab[1] = 4 * ((V - 1) // 4)
    if ignore == "third":
        lab[2::3] = IGNORE
    elif ignore == "all":
        lab[:] = IGNORE
    return lab


def ce_logits(family, rows, V, ld, dtype, seed, labels, n_valid=None):
    """[rows, ld] logits of a family.  Columns [V, ld) and the rows from n_valid on are NaN: the kernels must not let them
    reach a result."""
    g = gen(seed)
    x = 3.0 * torch.randn(rows, V, generator=g)
    on = (labels >= 0).nonzero().flatten()
    if family == "confident":
        top = x.max(1).values
        x[on, labels[on]] = top[on] + 20.0
    elif family == "wide":
        x = 160.0 * torch.rand(rows, V, generator=g) - 80.0
        x[:, 0] = 80.0
        x[:, V - 1] = -80.0
    elif family == "flat":
        x[:] = 1.5
    elif family == "masked":
        m = torch.rand(rows, V, generator=g) < 0.1
        m[:, 0] = False
        m[on, labels[on]] = False
        x[m] = -math.inf
    else:
        assert family == "plain", family
    full = torch.full((rows, ld), math.nan)
    full[:, :V] = x
    if n_valid is not None:
        full[n_valid:] = math.nan
    return full.to(dtype)


def _abs_finite(t):
    return torch.where(torch.isfinite(t), t.abs(), torch.zeros_like(t))


def ce_fwd_ref(x, V, labels, n_valid=None):
    """x [rows, ld], labels [rows]; rows from n_valid on do not exist.  -> dict: lse, lse_b [n_valid] (0 / unused on ignored
    rows), on [n_valid] bool, loss, loss_b (0-dim), count (int)."""
    n_valid = x.shape[0] if n_valid is None else n_valid
    xv, lab = x[:n_valid, :V].double(), labels[:n_valid].to(x.device)
    on = lab >= 0
    mx = xv.max(1, keepdim=True).values
    t = xv - mx
    e = torch.exp(t)
    s = e.sum(1)
    lse = mx[:, 0] + torch.log(s)
    e_s = ((2.0 * _abs_finite(t) + 3.0) * U32 * e).sum(1) + C_ACC * U32 * math.sqrt(V) * s
    e_lse = e_s / s + 2.0 * U32 * torch.log(s).abs() + U32 * lse.abs()
    xl = xv.gather(1, lab.clamp(min=0)[:, None])[:, 0]
    term = torch.where(on, lse - xl, torch.zeros_like(lse))
    e_term = torch.where(on, e_lse + U32 * term.abs(), torch.zeros_like(lse))
    n = int(on.sum())
    loss = term.sum()
    loss_b = SAFETY * (max(n - 1, 0) * U32 * term.abs().sum() + e_term.sum()) + TINY
    return dict(lse=torch.where(on, lse, torch.zeros_like(lse)), lse_b=SAFETY * e_lse + TINY, on=on, loss=loss, loss_b=loss_b,
                count=n)


def ce_bwd_ref(x, V, labels, lse, count, gscale, gscale_dev, dtype, n_valid=None):
    """lse [rows] f32 and count (a number) as handed to the kernel.  -> (dl, bound) [n_valid, V]; ignored rows are 0."""
    n_valid = x.shape[0] if n_valid is None else n_valid
    xv, lab = x[:n_valid, :V].double(), labels[:n_valid].to(x.device)
    on = (lab >= 0)[:, None]
    sc = f32(gscale) * (1.0 if gscale_dev is None else f32(gscale_dev)) / max(float(count), 1.0)
    t = xv - lse[:n_valid].double().to(x.device)[:, None]
    p = torch.exp(t)
    hot = torch.arange(V, device=x.device)[None, :] == lab[:, None]
    dl = torch.where(on, sc * (p - hot.double()), torch.zeros_like(p))
    b = abs(sc) * (2.0 * _abs_finite(t) + 3.0) * U32 * p + (4.0 * U32 + u_out(dtype)) * dl.abs()
    return dl, torch.where(on, SAFETY * b, torch.zeros_like(b)) + TINY


# ------------------------------------------------------------------ AdamW
ADAMW_N = (1, 2, 3, 4, 5, 1023, 10007, 524288, 524292, 2 * 524288 + 1203)
ADAMW_SWEEP = 512 * 256 * 4                 # elements of one trip of the capped grid
ADAMW_BETAS, ADAMW_EPS = (0.9, 0.999), 1e-6
ADAMW_HYPER = {"project": (4e-5, 1e-4), "big-lr": (1e-2, 0.0), "big-lr-wd": (1e-2, 1e-2)}          # name -> (lr, wd)
ADAMW_GRADS = ("randn", "zeros-third", "huge", "tiny", "gscale")


def adamw_grad(family, n, seed):
    """-> (g f32 [n], grad_scale)."""
    g = torch.randn(n, generator=gen(seed))
    if family == "zeros-third":
        g[::3] = 0.0
    elif family == "huge":
        g = 1e18 * g
    elif family == "tiny":
        g = 1e-20 * g
    else:
        assert family in ("randn", "gscale"), family
    return g, (1.0 / 1024 if family == "gscale" else 1.0)


def adamw_ref(p, g, m, v, lr, wd, step, gscale=1.0, coef=None, betas=ADAMW_BETAS, eps=ADAMW_EPS):
    """One step from the operands the kernel reads.  -> dict p, p_b, m, m_b, v, v_b (float64, the device of p)."""
    lr, wd, eps, b1, b2 = f32(lr), f32(wd), f32(eps), f32(betas[0]), f32(betas[1])
    bc1 = f32(1.0 - b1 ** step)
    bc2s = f32(math.sqrt(1.0 - b2 ** step))
    gs = f32(gscale) if coef is None else f32(f32(gscale) * f32(coef))
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gr = g * gs
    m1 = b1 * m + (1.0 - b1) * gr
    v1 = b2 * v + (1.0 - b2) * gr * gr
    e_m = U32 * ((b1 * m).abs() + 2.0 * ((1.0 - b1) * gr).abs() + m1.abs())
    e_v = U32 * (b2 * v + 4.0 * (1.0 - b2) * gr * gr + v1) + V_FLOOR
    p1 = p * (1.0 - lr * wd)
    r = torch.sqrt(v1)
    e_r = torch.minimum(e_v / (2.0 * r).clamp(min=1e-300), torch.sqrt(e_v)) + U32 * r
    den = r / bc2s + eps
    e_den = e_r / bc2s + U32 * r / bc2s + U32 * den
    q = (lr / bc1) * m1 / den
    e_q = (lr / bc1) * (e_m / den + m1.abs() * e_den / den ** 2) + 3.0 * U32 * q.abs()
    p2 = p1 - q
    e_p = 3.0 * U32 * p1.abs() + e_q + U32 * p2.abs()
    return dict(p=p2, p_b=SAFETY * e_p + TINY, m=m1, m_b=SAFETY * e_m + TINY, v=v1, v_b=SAFETY * e_v + TINY)


# ------------------------------------------------------------------ embeddings
def embed_ids(B, T, vocab, cls_id, sep_id, seed):
    """Text ids with repeats (a handful of distinct words, and word 0 as the padding the dense layout also sums), never the
    [CLS] / [SEP] ids."""
    pool = torch.tensor([w for w in range(vocab) if w not in (cls_id, sep_id)])
    few = pool[torch.randperm(pool.numel(), generator=gen(seed))[:max(3, min(pool.numel(), (B * T) // 3 + 1))]]
    ids = few[torch.randint(0, few.numel(), (B, T), generator=gen(seed + 1))]
    if T > 2:
        ids[:, -1] = 0
    return ids.long()


def embed_word_ids(text_ids, B, n_img, T, cls_id, sep_id):
    """[B, L] word id per position, -1 where the source is the image feature (emb_word_id)."""
    if n_img < 0:
        return text_ids.clone()
    w = torch.full((B, n_img + 2 + T), -1, dtype=torch.long)
    w[:, 0], w[:, n_img + 1] = cls_id, sep_id
    if T:
        w[:, n_img + 2:] = text_ids
    return w


def embed_types(L, n_img, type_override):
    if type_override >= 0:
        return torch.full((L,), type_override, dtype=torch.long)
    return (torch.arange(L) <= n_img + 1).long()


def embed_statement(text_ids, image, word, pos, typ, cls_id, sep_id, dtype, *, B, n_img, T, pos_offset=0, type_override=-1):
    """(src + type) + pos in f32 in that order, rounded to dtype: [B, L, H] on the CPU (IEEE additions: bit for bit what
    the kernel must store)."""
    H = word.shape[1]
    L = T if n_img < 0 else n_img + 2 + T
    wid = embed_word_ids(text_ids, B, n_img, T, cls_id, sep_id)
    src = word.float()[wid.clamp(min=0)]
    if n_img > 0:
        src[:, 1:1 + n_img] = image.float()
    ty = embed_types(L, n_img, type_override)
    out = (src + typ.float()[ty][None]) + pos.float()[pos_offset:pos_offset + L][None]
    assert out.shape == (B, L, H)
    return out.to(dtype)


def batch_sum_ref(g):
    """Ordered f32 sum over dim 0 of g [B, ...] (a slice of dout: any columns of a position row).  -> (ref, bound)."""
    g = g.double()
    s = g.sum(0)
    return s, SAFETY * (C_ACC * U32 * math.sqrt(g.shape[0]) * g.abs().sum(0) + U32 * s.abs()) + TINY


def embed_bwd_ref(dout, wid, valid, word_prior, *, n_img, pos_rows, type_rows, pos_offset=0, type_override=-1):
    """dout [B, L, H] (positions that are not materialised hold anything: ``valid`` [B, L] bool masks them), wid [B, L].
    -> dict: dword, dword_b [vocab, H], hits [vocab]; dpos, dpos_b [pos_rows, H]; dtype, dtype_b [type_rows, H];
    pos_used [pos_rows] / type_used [type_rows] bool (rows outside must be exactly 0)."""
    B, L, H = dout.shape
    g = dout.double() * valid[:, :, None].double()
    a = g.abs()
    prior = word_prior.double()
    vocab = prior.shape[0]
    flat = (wid * valid).clamp(min=0).reshape(-1)
    w_on = ((wid >= 0) & valid).reshape(-1)
    idx = flat[w_on]
    dword = prior.clone().index_add_(0, idx, g.reshape(-1, H)[w_on])
    asum = prior.abs().index_add_(0, idx, a.reshape(-1, H)[w_on])
    hits = torch.zeros(vocab, dtype=torch.long).index_add_(0, idx, torch.ones_like(idx))
    out = dict(dword=dword, dword_b=SAFETY * hits[:, None].double() * U32 * asum + TINY, hits=hits)
    nb = valid.sum(0).clamp(min=1).double()[:, None]                                          # terms of a position row
    dpos, dpos_b = torch.zeros(pos_rows, H, dtype=torch.float64), torch.full((pos_rows, H), TINY, dtype=torch.float64)
    dpos[pos_offset:pos_offset + L] = g.sum(0)
    dpos_b[pos_offset:pos_offset + L] = SAFETY * (C_ACC * U32 * nb.sqrt() * a.sum(0) + U32 * g.sum(0).abs()) + TINY
    used = torch.zeros(pos_rows, dtype=torch.bool)
    used[pos_offset:pos_offset + L] = True
    out.update(dpos=dpos, dpos_b=dpos_b, pos_used=used)
    ty = embed_types(L, n_img, type_override)
    dty, dty_b = torch.zeros(type_rows, H, dtype=torch.float64), torch.full((type_rows, H), TINY, dtype=torch.float64)
    tused = torch.zeros(type_rows, dtype=torch.bool)
    for r in ([type_override] if type_override >= 0 else [0, 1]):
        sel = ty == r
        n = max(int(valid[:, sel].sum()), 1)
        s = g[:, sel].sum((0, 1))
        dty[r] = s
        dty_b[r] = SAFETY * (C_ACC * U32 * math.sqrt(n) * a[:, sel].sum((0, 1)) + U32 * s.abs()) + TINY
        tused[r] = True
    out.update(dtype=dty, dtype_b=dty_b, type_used=tused)
    return out


# ------------------------------------------------------------------ column sums
COLSUM_M = (1, 63, 64, 65, 129, 3000, 8197)
COLSUM_N = (1, 3, 4, 5, 255, 257, 388)
COLSUM_LD = ("ld==N", "ld>N,ld%4==0", "ld>N,ld%4!=0")
COLSUM_SLICES = 128


def colsum_ld(N, kind):
    if kind == "ld==N":
        return N
    ld = (N + 3) // 4 * 4 + 4
    return ld if kind == "ld>N,ld%4==0" else ld + 1


def colsum_x(family, M, N, ld, dtype, seed):
    """The wide [M, ld] tensor (columns >= N are NaN); the operand is its view [:, :N], whose base stays 16-byte aligned."""
    x = torch.randn(M, N, generator=gen(seed))
    if family == "offset":
        x = x + 30.0
    else:
        assert family == "randn", family
    wide = torch.full((M, ld), math.nan)
    wide[:, :N] = x
    return wide.to(dtype)


def colsum_ref(x, prev=None):
    """x [M, N] (the view).  -> (ref, bound) [N]; prev: the output's previous content under accumulate."""
    x = x.double()
    ref = x.sum(0)
    bound = C_ACC * U32 * math.sqrt(x.shape[0]) * x.abs().sum(0)
    if prev is not None:
        ref = ref + prev.double().to(x.device)
        bound = bound + U32 * ref.abs()
    return ref, bound + TINY


# ------------------------------------------------------------------ elementwise
UNARY_N = (1, 255, 257, 8192 * 256 + 257)
UNARY_SPECIAL = (0.0, -0.0, 8.0, -8.0, 40.0, -40.0)


def unary_x(n, dtype, seed):
    x = 2.0 * torch.randn(n, generator=gen(seed))
    k = min(n, len(UNARY_SPECIAL))
    x[:k] = torch.tensor(UNARY_SPECIAL[:k])
    return x.to(dtype)


def unary_ref(op, a, b, dtype):
    """op: gelu(x) | tanh(x) | gelu_bwd(x, dy) | tanh_bwd(y, dy).  -> (ref, bound)."""
    a = a.double()
    uo = u_out(dtype)
    if op == "gelu":
        r = gelu64(a)
        e = ERFC_ABS * a.abs() + (4 * U32 + uo) * r.abs()
    elif op == "tanh":
        r = torch.tanh(a)
        e = (4 * U32 + uo) * r.abs()
    elif op == "gelu_bwd":
        b = b.double()
        r = b * gelu_grad64(a)
        e = ERFC_ABS * b.abs() + (4 * U32 + uo) * r.abs()
    else:
        assert op == "tanh_bwd", op
        b = b.double()
        r = b * (1.0 - a * a)
        e = U32 * b.abs() * (a * a + 2.0 * (1.0 - a * a).abs()) + uo * r.abs()
    return r, SAFETY * e + TINY


CAST_N = (1, 2, 3, 5, 1003, 4 * 8192 * 256 + 4 * 300 + 3)


def cast_specials():
    """f32 values whose bf16 rounding is decided by a rule, each with both signs: ties (to even, up and down), values just
    beside a tie, +-inf, NaN, the largest finite f32 (rounds to inf), f32 denormals.  -> (values, is_denormal)."""
    ties = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -23,
            255.0 + 0.5, 3.3895313892515355e38, 65280.0 + 128.0]
    big = [math.inf, 3.4028234663852886e38, 1.1754943508222875e-38]
    den = [2.0 ** -149, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, 2.0 ** -127, 2.0 ** -126 - 2.0 ** -149, 2.0 ** -130 + 2.0 ** -140]
    pos = torch.tensor(ties + big + den, dtype=torch.float64)
    v = torch.cat([pos, -pos, torch.tensor([math.nan, -math.nan], dtype=torch.float64)]).float()
    is_den = (v.abs() < 2.0 ** -126) & (v != 0)
    return v, is_den
