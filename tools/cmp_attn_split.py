"""A/B of the location-attention kernels at bench-like shapes: run with OS2S_ATTN_SPLIT=0 and =1
(read when the library is loaded; the option attn_decoder.attn_split), each run dumps its outputs; `cmp` compares the two dumps.
usage: cmp_attn_split.py run <out.pt> | cmp <a.pt> <b.pt>"""
import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

if sys.argv[1] == "cmp":
  a, b = torch.load(sys.argv[2]), torch.load(sys.argv[3])
  for k in a:
    x, y = a[k].float(), b[k].float()
    rel = float((x - y).norm() / (y.norm() + 1e-20))
    print("%-12s rel-L2 %.3e  max|d| %.3e  norm %.3e %s" % (k, rel, float((x - y).abs().max()), float(y.norm()),
                                                          "  <-- " if rel > 2e-2 else ""))
  sys.exit(0)

from openseq2seq_amd import _lib, capi
dev = torch.device("cuda:0")
B, T, S, L, H, M, U, mode, K, F = 32, 120, 200, 2, 1024, 1024, 128, 2, 32, 32
g = torch.Generator().manual_seed(0)
rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc)
bf = lambda t: t.to(torch.bfloat16).to(dev)
kc = [M + H, 2 * H]
wcat = [bf(rn(4 * H, kc[l], sc=0.35 / math.sqrt(kc[l]))) for l in range(L)]
dec = capi.AttnDecoder(B, T, S, L, H, M, U, mode, dev, use_bias=True, loc_k=K, loc_f=F, out_keep=0.9,
                       out_seeds=(1, 2))
wq = bf(rn(U, H, sc=1 / math.sqrt(H)))
dec.set_params(wcat, wq, rn(U, sc=0.2).to(dev), bias=[None] + [rn(4 * H, sc=0.1).to(dev)] * (L - 1),
               g=torch.ones(1, device=dev), b=rn(U, sc=0.1).to(dev), conv_w=rn(K, F, sc=0.5).to(dev),
               conv_b=rn(F, sc=0.1).to(dev), dense_w=rn(F, U, sc=0.3).to(dev))
src_len = torch.randint(S // 3, S + 1, (B,), generator=g, dtype=torch.int32)
src_len[0] = S
tgt_len = torch.randint(T // 3, T + 1, (B,), generator=g, dtype=torch.int32)
tgt_len[0] = T
mem = rn(B, S, M)
mem = mem * (torch.arange(S)[None, :, None] < src_len[:, None, None])
wmem = bf(rn(U, M, sc=1 / math.sqrt(M)))
values = bf(mem)
keys = (values.float() @ wmem.float().t()).to(torch.bfloat16)
dec.set_inputs(bf(rn(B, T, 4 * H, sc=0.7)), keys, values, src_len.to(dev), tgt_len.to(dev))
dec.forward()
z = lambda *s: torch.zeros(*s, device=dev)
dv, dcw, dcb, ddw = z(U), z(K, F), z(F), z(F, U)
out = dec.backward([w.t().contiguous() for w in wcat], wq.t().contiguous(), dy_top=bf(rn(B, T, H)),
                   dctx_ext=bf(rn(B, T, M)), dv=dv, dg=z(1), dconv_w=dcw, dconv_b=dcb, ddense_w=ddw)
torch.cuda.synchronize()
dump = dict(y_top=dec.y_top, ctx=dec.ctx, align=dec.align_seq, cum=dec.cum_seq, dg0=out["dg"][0], dg1=out["dg"][1],
            dmem=out["dmem"], dkeys=out["dkeys"], dq=out["dq_seq"], dv=dv, dconv_w=dcw, dconv_b=dcb, ddense_w=ddw)
torch.save({k: v.detach().float().cpu() for k, v in dump.items()}, sys.argv[2])
print("saved", sys.argv[2], "split = %d" % _lib.get_option("attn_decoder.attn_split"))
