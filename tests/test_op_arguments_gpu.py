"""Every native op checks its tensor arguments (csrc/bindings/tensor_args.h) before anything is launched.

One table entry per registered ``dtfe::`` op: a valid call at the smallest shape the op accepts, and
mutations of one argument at a time - the wrong dtype, one element short, not contiguous, the wrong
device.  The valid call returns; every mutated call raises RuntimeError naming the op and the argument,
and leaves every output as it was.

A refused call is harmless even where a check were missing: a wrong dtype has at least as many bytes, a
short tensor is a view of a full-size buffer, a strided one a view of a buffer twice the size, and the
wrong-device tensor is pinned host memory, which the device can address."""
import pytest
import torch

import dtfe.ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def f32(*s):
    return torch.randn(*s, device=DEV)


def b16(*s):
    return torch.randn(*s, device=DEV).to(torch.bfloat16)


def u8(*s, hi=4):
    return torch.randint(0, hi, s, dtype=torch.uint8, device=DEV)


def i32(*s, hi=1):
    return torch.randint(0, hi, s, dtype=torch.int32, device=DEV)


def i64(*s):
    return torch.zeros(*s, dtype=torch.int64, device=DEV)


# a dtype no accessor takes in place of the key, with at least as many bytes per element
WRONG = {torch.float32: torch.int32, torch.bfloat16: torch.float32, torch.uint8: torch.float32,
         torch.int32: torch.int64, torch.int64: torch.float64}


def mutate(t, kind):
    """(the argument to pass, the buffer behind it)"""
    if kind == "dtype":
        m = torch.zeros(t.shape, dtype=WRONG[t.dtype], device=DEV)
        return m, m
    if kind == "short":  # one element short: a view of a buffer of the full size
        full = t.clone().reshape(-1)
        return full[:full.numel() - 1], full
    if kind == "strided":  # the same shape over every second element of a buffer twice the size
        full = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=DEV)
        return full[..., ::2], full
    if kind == "pinned":  # not on the op's device, yet device-addressable
        m = torch.zeros(t.shape, dtype=t.dtype).pin_memory()
        return m, m
    raise KeyError(kind)


CASES = {}


def case(name, make, order, outs=(), muts=""):
    """make(): the named arguments of a valid call; order: the op's positional arguments - a string names an
    entry of make(), a list is a list argument, anything else is passed as it stands; outs: the tensors the
    op writes; muts: "argument:kind" words."""
    CASES[name] = (make, order, tuple(outs.split()) if isinstance(outs, str) else outs, muts.split())


def call(name, args):
    make, order, _outs, _muts = CASES[name]

    def res(x):
        if isinstance(x, str):
            return args[x]
        if isinstance(x, list):
            return [res(y) for y in x]
        return x

    return getattr(ops.require(), name)(*[res(x) for x in order])


# ------------------------------------------------------------------- gemm
case("gemm", lambda: dict(A=f32(64, 64), B=f32(64, 64), out=f32(64, 64), bias=f32(64), aux=f32(64, 64), out2=f32(64, 64)),
     ["A", 0, 64, "B", 0, 64, 64, 64, 64, "out", 64, "bias", 0, 0, 1.0, 0.0, False, 1, 0, "aux", 64, 1, -1, 1.0, 0, None,
      None, None, 0, 0, 0, "out2", 64, False, None, None, None],
     "out out2", "A:short A:strided B:short out:short out:dtype out:strided bias:short bias:dtype aux:short out2:short out2:dtype")
case("wgrad_tallk", lambda: dict(A=f32(4, 8), B=f32(4, 64), out=f32(8, 64), bias=f32(64),
                                 ws=f32(ops.tallk_ws_floats(8, 64, 2))),
     ["A", 8, "B", 64, 8, 64, 4, "out", 64, "bias", "ws", 2, 1.0],
     "out bias ws", "A:short A:dtype B:short out:short out:dtype out:strided bias:short ws:dtype")
case("colsum", lambda: dict(x=f32(4, 16), db=f32(16)), ["x", 4, 16, 16, "db", 1.0],
     "db", "x:short x:dtype x:strided db:short db:dtype")

# ------------------------------------------------------------------- conv
G = [2, 16, 16, 16, 32, 8, 8, 3, 3, 2, 1]  # B, H, W, C, Cout, OH, OW, KH, KW, stride, pad
case("conv_fwd", lambda: dict(x=b16(2, 16, 16, 16), w=b16(32, 3, 3, 16), bias=f32(32), y=b16(2, 8, 8, 32)),
     ["x", "w", "bias", "y", None, *G, False, 1],
     "y", "x:short w:short w:dtype bias:short bias:dtype y:short y:dtype y:strided")
case("conv_dgrad", lambda: dict(dy=b16(2, 8, 8, 32), wt=b16(16, 3, 3, 32), dx=b16(2, 16, 16, 16)),
     ["dy", "wt", "dx", *G, None, None, None],
     "dx", "dy:short wt:short wt:dtype dx:short dx:dtype dx:strided")
case("conv_wgrad", lambda: dict(dz=b16(2, 8, 8, 32), x=b16(2, 16, 16, 16), dw=f32(32, 3, 3, 16), db=f32(32)),
     ["dz", "x", "dw", "db", *G, 0.5],
     "dw db", "dz:short x:short x:dtype dw:short dw:dtype db:short db:dtype")
IG = [8, 8, 64, 8, 8, 64, 3, 3, 1, 1]  # SH, SW, CS, OH, OW, N, KH, KW, stride, pad
case("imgconv", lambda: dict(src=b16(2, 8, 8, 64), w=b16(64, 9, 64), bias=f32(64), y=b16(2, 8, 8, 64)),
     ["src", None, None, "w", "bias", "y", None, None, 2, *IG, False, 1, False],
     "y", "src:short src:dtype w:short w:dtype bias:short bias:dtype y:short y:dtype y:strided")
case("imgwgrad", lambda: dict(src=b16(6, 8, 8, 64), dy=b16(6, 8, 8, 64), dw=f32(64, 9, 64), db=f32(64),
                              ws=torch.zeros(ops.wgrad_ws_floats(64, 9 * 64), device=DEV)),
     ["src", "dy", None, None, "dw", "db", 6, *IG, 0.5, "ws"],
     "dw db ws", "src:short src:dtype dy:short dy:dtype dw:short dw:dtype db:short ws:dtype")


def _deferred_reduce():  # the descriptor and workspace that a deferred weight gradient leaves behind
    a = dict(src=b16(256, 8, 8, 64), dy=b16(256, 8, 8, 64), dw=f32(64, 9, 64), db=f32(64),
             ws=torch.zeros(ops.wgrad_ws_floats(64, 9 * 64), device=DEV))
    a["desc"] = list(ops.require().imgwgrad(a["src"], a["dy"], None, None, a["dw"], a["db"], 256, *IG, 0.5, a["ws"], 0,
                                            None, 0.001, True))
    assert len(a["desc"]) == 6
    return a


case("wgrad_reduce_group", _deferred_reduce, [["ws"], ["dw"], ["db"], [0.5], "desc"],
     "dw db", "ws:dtype dw:short dw:dtype db:short db:dtype")


def _conv1(B=256):
    return dict(images=u8(300, 784, hi=256), labels_src=i32(300, hi=10), counter=i64(1), done=i32(1), labels_dst=i32(B),
                x=b16(B, 28, 28), w=b16(32, 25), bias=f32(32), y=b16(B, 14, 14, 32), argmax=u8(B, 14, 14, 32),
                zero=f32(4), w2=b16(64, 25, 32), bias2=f32(64), p2=b16(B, 7, 7, 64), a2=u8(B, 7, 7, 64))


CONV1 = ["images", "labels_src", 0, "counter", "done", "labels_dst", "x", "w", "bias", "y", "argmax", ["zero"]]
CONV1_OUTS = "counter done labels_dst x y argmax zero"
CONV1_MUTS = ("labels_src:short labels_src:dtype counter:dtype done:dtype labels_dst:short x:dtype w:short w:dtype "
              "bias:short y:short y:dtype argmax:short argmax:dtype zero:strided")
case("conv1_gather_fwd", _conv1, CONV1, CONV1_OUTS, CONV1_MUTS)
case("conv12_gather_fwd", _conv1, CONV1 + ["w2", "bias2", "p2", "a2"], CONV1_OUTS + " p2 a2",
     CONV1_MUTS + " w2:short w2:dtype bias2:short bias2:dtype p2:short p2:dtype a2:short a2:dtype")
case("unpool_f32", lambda: dict(g=f32(2, 2, 2, 8), argmax=u8(2, 2, 2, 8), out=f32(2, 4, 4, 8)),
     ["g", "argmax", "out", 2, 2, 2, 8], "out", "g:short argmax:short argmax:dtype out:short out:dtype out:strided")
case("conv1_wgrad_pooled_f32", lambda: dict(dp=f32(3, 8, 8, 32), argmax=u8(3, 8, 8, 32), x=f32(3, 16, 16),
                                            dw=f32(32, 3, 3), db=f32(32), ws=f32(3 * (32 * 25 + 32))),
     ["dp", "argmax", "x", "dw", "db", "ws", 3, 16, 16, 3, 0.5],
     "dw db ws", "argmax:short argmax:dtype x:short dw:short dw:dtype db:short ws:dtype")
case("transpose_taps_f32", lambda: dict(w=f32(4, 9, 8), out=f32(8, 9, 4)), ["w", "out", 4, 9, 8],
     "out", "out:short out:dtype out:strided")

# ------------------------------------------------------------------- heads
case("head_xent_f32", lambda: dict(h=f32(2, 8), w=f32(10, 8), b=f32(10), labels=i32(2, hi=10), dz=f32(2, 8), dl=f32(2, 10),
                                   loss_sum=f32(1), correct=i32(1), logits=f32(2, 10)),
     ["h", "w", "b", "labels", "dz", "dl", "loss_sum", "correct", "logits", 0.5, 1.0, None],
     "dz dl loss_sum correct logits", "w:dtype b:short labels:short labels:dtype dz:short dl:short dl:dtype "
     "loss_sum:dtype correct:dtype logits:short")
case("head_xent", lambda: dict(h=b16(4, 1024), w=b16(10, 1024), b=f32(10), labels=i32(4, hi=10), dz=b16(4, 1024),
                               dl=b16(4, 16), loss_sum=f32(1), correct=i32(1), logits=f32(4, 10)),
     ["h", "w", "b", "labels", "dz", "dl", "loss_sum", "correct", "logits", 0.25, 1.0],
     "dz dl loss_sum correct logits", "h:dtype w:short w:dtype b:short labels:short labels:dtype dz:short dz:dtype "
     "dl:dtype dl:strided loss_sum:dtype correct:dtype logits:short logits:dtype")
case("head_wgrad", lambda: dict(dl=b16(4, 16), h=b16(4, 64), dw=f32(10, 64), db=f32(10)),
     ["dl", "h", "dw", "db", 10, 0.5], "dw db", "dl:dtype dl:strided h:dtype dw:dtype db:short db:dtype")
case("dense_head", lambda: dict(feat=b16(4, 16), w=f32(10, 16), bias=f32(10), y=f32(4, 10), logits=f32(4, 10),
                                loss_sum=f32(1), correct=i32(1), dw=f32(10, 16), db=f32(10), dfeat=b16(4, 16)),
     ["feat", "w", "bias", "y", "logits", "loss_sum", "correct", "dw", "db", "dfeat", 0.25],
     "logits loss_sum correct dw db dfeat", "feat:strided w:dtype bias:short y:short y:dtype logits:short loss_sum:dtype "
     "correct:dtype dw:short dw:dtype db:short dfeat:short dfeat:dtype")
case("softmax_xent", lambda: dict(logits=f32(4, 10), labels_i=i32(4, hi=10), dlogits=f32(4, 10), loss_rows=f32(4),
                                  loss_sum=f32(1), correct=i32(1), probs=f32(4, 10)),
     ["logits", "labels_i", None, 0.25, "dlogits", "loss_rows", "loss_sum", "correct", "probs"],
     "dlogits loss_rows loss_sum correct probs", "logits:strided labels_i:short labels_i:dtype dlogits:short dlogits:dtype "
     "loss_rows:short loss_sum:dtype correct:dtype probs:short")
case("gan_loss", lambda: dict(d_real=f32(4), d_fake=f32(4), gen_loss=f32(1), disc_loss=f32(1), dz_real_disc=f32(4),
                              dz_fake_disc=f32(4), dz_fake_gen=f32(4)),
     ["d_real", "d_fake", "gen_loss", "disc_loss", "dz_real_disc", "dz_fake_disc", "dz_fake_gen", 0.0],
     "gen_loss disc_loss dz_real_disc dz_fake_disc dz_fake_gen", "d_fake:short d_fake:dtype gen_loss:dtype disc_loss:dtype "
     "dz_real_disc:short dz_fake_disc:short dz_fake_gen:short dz_fake_gen:dtype")
case("gan_disc_head", lambda: dict(d1=f32(4, 8), w=f32(8), b=f32(1), p=f32(4), dlog=f32(4), dlog_g=f32(2), gw=f32(8),
                                   gb=f32(1), dd1=f32(4, 8), ddf=f32(2, 8), gen_loss=f32(1), disc_loss=f32(1),
                                   ws=torch.zeros(ops.gan_head_ws_floats(2, 8), device=DEV)),
     ["d1", "w", "b", "p", "dlog", "dlog_g", "gw", "gb", "dd1", "ddf", "gen_loss", "disc_loss", "ws", 0.0],
     "p dlog dlog_g gw gb dd1 ddf gen_loss disc_loss ws", "w:short w:dtype p:short dlog:short dlog_g:short gw:short "
     "dd1:short dd1:dtype ddf:short gen_loss:dtype ws:short ws:dtype")
case("mse_sigmoid", lambda: dict(y=f32(8), t=f32(8), loss=f32(1), dz=f32(8), ws=torch.zeros(132, device=DEV)),
     ["y", "t", "loss", "dz", "ws"], "loss dz ws", "t:short t:dtype loss:dtype dz:short dz:dtype ws:short ws:dtype")


# -------------------------------------------------------------- optimizer
def _opt(n=64):
    a = dict(p=f32(n), done=i32(1), g=f32(n))
    a["st"] = ops.opt_state(ops.OPT_SGD, a["p"], [[0, n, 1, 1, 0, 0]], [[0, 0, 0, 0, 0, 0, n]], a["done"])
    return a


case("apply_gradients", _opt, ["st", "g", None, 1.0, 0.1, 0], "p done", "g:short g:dtype g:strided")
case("apply_gradients_group", _opt, [["st"], "g", None, 1.0, [0.1], [0]], "p done", "g:short g:dtype g:strided")
case("lr_schedule_pack", lambda: dict(like=f32(1)), [0, [], [], 0.1, 0.0, 0, 0.0, 0, 0.0, "like"])
case("epoch_signal", lambda: dict(ctr=i32(1)), ["ctr"], "ctr", "ctr:dtype")


def _norm(n=10000):  # two chunks
    g = f32(n)
    return dict(g=g, t=g, plan=ops.grad_norm_plan([(0, n)], g), partials=f32(2), ticket=i32(1), out=f32(2), scale=f32(1))


case("grad_sumsq", _norm, ["g", None, 1.0, 1.0, "plan", "partials", "ticket", "out"],
     "partials ticket out", "g:dtype plan:dtype partials:short partials:dtype ticket:dtype out:short out:dtype")
case("scale_", _norm, ["t", "scale", "plan"], "t", "t:dtype scale:short scale:dtype plan:dtype")


def _lars(n=100):
    p = f32(n)
    plan, segs, limit = ops.layer_trust_plan([(0, 0, n)], p)
    return dict(p=p, g=f32(n), plan=plan, segs=segs, limit=limit, wd=torch.zeros(1, device=DEV), partials=f32(2),
                ticket=i32(1), sums=f32(1, 2), trust=f32(1))


case("layer_trust", _lars, ["p", "g", None, 1.0, "plan", "segs", "limit", "wd", 0.001, 0.0, None, "partials", "ticket",
                            "sums", "trust"],
     "partials ticket sums trust", "p:short g:short g:dtype plan:dtype segs:dtype wd:dtype partials:short partials:dtype "
     "ticket:dtype sums:short sums:dtype trust:short trust:dtype")
case("eval_metrics", lambda: dict(logits=f32(4, 10), labels=i32(4, hi=10), state=ops.eval_state(DEV, 4), ws=i32(8),
                                  ticket=i32(1)),
     ["logits", "labels", 1, "state", None, "ws", "ticket"],
     "state ws ticket", "labels:short labels:dtype state:short state:dtype ws:short ws:dtype ticket:dtype")


# ------------------------------------------------------------ data movers
def _rows(D=16):
    return dict(src=u8(8, D, hi=256), dst=f32(4, D) if D == 16 else f32(4, 4, 4, 3), idx=i32(4, hi=8),
                labels_src=i32(8, hi=10), labels_dst=i32(4), counter=i64(1), done=i32(1), zero=f32(4), mean=f32(3),
                inv_std=f32(3))


ROWS_OUTS = "dst labels_dst counter done zero"
ROWS_MUTS = ("dst:dtype dst:strided idx:short idx:dtype labels_src:short labels_src:dtype labels_dst:short "
             "labels_dst:dtype counter:dtype done:dtype zero:strided")
case("gather_rows", _rows, ["src", "dst", "idx", "labels_src", "labels_dst", 0, "counter", "done", ["zero"]],
     ROWS_OUTS, ROWS_MUTS)
case("augment_rows", lambda: _rows(48), ["src", "dst", 4, 4, 3, 1, True, "mean", "inv_std", "idx", "labels_src",
                                         "labels_dst", 0, "counter", "done", ["zero"]],
     ROWS_OUTS, ROWS_MUTS + " mean:short mean:dtype inv_std:short")
case("uniform_fill", lambda: dict(out=f32(16), counter=i64(1), done=i32(1), copy_src=f32(8), copy_dst=f32(8)),
     ["out", 0.0, 1.0, 0, "counter", "done", "copy_src", "copy_dst"],
     "out counter done copy_dst", "out:dtype out:strided counter:dtype done:dtype copy_src:dtype copy_dst:short copy_dst:dtype")
case("cast_", lambda: dict(src=f32(16), dst=b16(16)), ["src", "dst"], "dst", "src:strided dst:short dst:dtype dst:strided")
case("seq_stage", lambda: dict(x=f32(2, 12), xh=f32(3, 2, 12), ysrc=f32(2, 5), ydst=f32(2, 5), zero=f32(4)),
     ["x", "xh", 3, 4, "ysrc", "ydst", ["zero"]],
     "xh ydst zero", "x:short x:dtype xh:dtype ysrc:dtype ydst:short ydst:dtype zero:strided")
case("act_grad", lambda: dict(dy=f32(8), y=f32(8), dz=f32(8)), ["dy", "y", "dz", 1],
     "dz", "dy:strided y:short y:dtype dz:short dz:dtype")
case("bias_act", lambda: dict(x=f32(4, 16), bias=f32(16), out=f32(4, 16)), ["x", "bias", "out", 1, 1.0, 0, None],
     "out", "bias:short bias:dtype out:short out:dtype out:strided")

# ------------------------------------------------------------------- lstm
case("lstm_cell_fwd", lambda: dict(gates=f32(2, 32), act=f32(2, 32), c_prev=f32(2, 8), c=f32(2, 8), h_out=f32(2, 8)),
     ["gates", "act", "c_prev", "c", "h_out", 8, 1.0],
     "act c h_out", "gates:short gates:dtype act:short act:strided c_prev:short c:dtype h_out:short h_out:dtype h_out:strided")
case("lstm_cell_bwd", lambda: dict(act=f32(2, 32), c_prev=f32(2, 8), c=f32(2, 8), dh=f32(2, 8), dc_next=f32(2, 8),
                                   dgates=f32(2, 32), dc_prev=f32(2, 8)),
     ["act", "c_prev", "c", "dh", None, "dc_next", "dgates", "dc_prev"],
     "dgates dc_prev", "act:short c_prev:short dh:short dh:dtype dc_next:short dgates:short dgates:dtype dc_prev:short")
# H = 8 is not a shape the whole-sequence kernels cover: both return False
case("lstm_seq_fwd", lambda: dict(xh=f32(2, 2, 12), K=f32(12, 32), bias=f32(32), act=f32(2, 2, 32), c=f32(2, 2, 8),
                                  hT=f32(2, 8)),
     ["xh", "K", "bias", 1.0, "act", "c", "hT"], "xh act c hT", "K:short K:dtype bias:short act:short act:dtype c:short hT:dtype")
case("lstm_seq_bwd", lambda: dict(K=f32(12, 32), act=f32(2, 2, 32), c=f32(2, 2, 8), dhT=f32(2, 8), dg=f32(2, 2, 32)),
     ["K", "act", "c", "dhT", "dg", 4], "dg", "K:short act:short dhT:short dhT:dtype dg:short dg:dtype")


# ------------------------------------------------------------------- norm
def _bn(y=(2, 4, 4, 16), dy=(2, 4, 4, 16)):  # y / dy: full size, pooled [2][2][2][16] or averaged [2][16]
    X = (2, 4, 4, 16)
    return dict(x=b16(*X), dy=b16(*dy), y=b16(*y), res=b16(*X), out=b16(*X), dx=b16(*X), dres=b16(*X), stats=f32(2, 16),
                gamma=f32(16), beta=f32(16), mean=f32(16), invstd=f32(16), moving_mean=f32(16), moving_var=f32(16).abs(),
                dgamma=f32(16), dbeta=f32(16), mask_out=u8(64), am=u8(2, 2, 2, 16, hi=9), dp=b16(2, 2, 2, 16))


def _pooled():
    return _bn(y=(2, 2, 2, 16), dy=(2, 2, 2, 16))


def _averaged():
    return _bn(y=(2, 16), dy=(2, 16))


case("bn_stats", _bn, ["x", "stats"], "stats", "x:dtype x:strided stats:short stats:dtype")
case("bn_apply", _bn, ["x", "stats", "gamma", "beta", "mean", "invstd", "moving_mean", "moving_var", 1e-3, 0.99, 1, "res",
                       1, 4, 4, "out", "mask_out"],
     "mean invstd moving_mean moving_var out mask_out", "gamma:short gamma:dtype beta:short mean:short invstd:short "
     "moving_mean:short moving_var:dtype res:dtype res:strided out:short out:dtype out:strided mask_out:short mask_out:dtype")
case("bn_infer", _bn, ["x", "gamma", "beta", "moving_mean", "moving_var", 1e-3, 1, "res", 1, 4, 4, "out"],
     "out", "gamma:short beta:dtype moving_mean:short moving_var:short res:dtype out:short out:dtype")
case("bn_bwd_stats", _bn, ["dy", "y", "x", "mean", "invstd", "stats", 1],
     "stats", "dy:short dy:dtype y:short y:dtype mean:short mean:dtype invstd:short stats:short")
case("bn_bwd_apply", _bn, ["dy", "y", "x", "mean", "invstd", "gamma", "stats", 1, "dx", "dres", "dgamma", "dbeta"],
     "dx dres dgamma dbeta", "dy:short gamma:short dx:short dx:dtype dx:strided dres:short dgamma:short dgamma:dtype dbeta:short")
case("bn_relu_pool3", _pooled, ["x", "stats", "gamma", "beta", "mean", "invstd", "moving_mean", "moving_var", 1e-3, 0.99,
                                "y", "am"],
     "mean invstd moving_mean moving_var y am", "stats:short gamma:short beta:short mean:short y:dtype am:short am:dtype")
case("pool3_bn_bwd", _pooled, ["dp", "am", "x", "mean", "invstd", "gamma", "beta", "stats", "dx", "dgamma", "dbeta"],
     "stats dx dgamma dbeta", "dp:dtype am:short am:dtype mean:short gamma:short stats:short dx:short dx:dtype dgamma:short "
     "dbeta:dtype")
case("shortcut_grad_add", lambda: dict(g=b16(2, 2, 2, 16), dx=b16(2, 4, 4, 8)), ["g", "dx", 2],
     "dx", "g:dtype g:strided dx:dtype dx:strided")
# y:pinned is the suite's one wrong-device case: with one visible GPU there is no second device to take a tensor from
case("gap_fwd", _averaged, ["x", "y"], "y", "x:dtype x:strided y:short y:dtype y:strided y:pinned")
case("gap_bwd", _averaged, ["dy", "dx"], "dx", "dy:short dy:dtype dx:dtype dx:strided")
case("maxpool3_fwd", _pooled, ["x", "y", "am"], "y am", "x:dtype y:dtype y:strided am:short am:dtype")
case("maxpool3_bwd", _pooled, ["dy", "am", "dx"], "dx", "dy:dtype am:short am:dtype dx:dtype dx:strided")

# ops with no tensor argument to check
NO_TENSORS = {"lstm_status", "lstm_last_split", "gan_head_ws_floats", "ema_swap"}


def _fresh(name):
    torch.manual_seed(11)
    return CASES[name][0]()


def test_every_registered_op_has_an_entry():
    ops.require()
    names = {n.split("::")[1].split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith("dtfe::")}
    names = {n for n in names if not n.startswith(("ps_", "ipc_", "rccl_"))} - NO_TENSORS
    assert names == set(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_the_valid_call_is_accepted(name):
    out = call(name, _fresh(name))
    torch.cuda.synchronize()
    assert out is None or isinstance(out, (bool, list, torch.Tensor))


MUTATIONS = [(name, m) for name in CASES for m in CASES[name][3]]


@pytest.mark.parametrize("name,mut", MUTATIONS, ids=["%s-%s" % nm for nm in MUTATIONS])
def test_a_mutated_argument_is_refused_before_anything_is_written(name, mut):
    arg, kind = mut.split(":")
    args = _fresh(name)
    args[arg], backing = mutate(args[arg], kind)
    watched = [args[o] for o in CASES[name][2] if o != arg] + [backing]
    before = [w.clone() for w in watched]
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError) as e:
        call(name, args)
    msg = str(e.value)
    del e  # (its traceback holds this frame: kept, the two are a cycle that keeps every tensor here alive)
    assert name in msg and arg in msg, msg
    torch.cuda.synchronize()
    for w, b in zip(watched, before):
        assert torch.equal(w.view(torch.uint8), b.view(torch.uint8))
