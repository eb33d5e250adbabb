"""Cold random gather from int4 / int8 row-wise, bf16 and fp32 tables.

The shape of bench_cold.py (213k one-hot rows, width 128, 16 id pools so no
call repeats the previous call's rows) on a table large enough to defeat L2
and the Infinity Cache, with the table kinds alternated inside every repeat so
that drift hits all of them alike.  Prints rows/s per repeat, the median, the
spread (max - min) and the table bytes fetched per second.

  python tools/bench_q8.py                        # int8, bf16, fp32 + quantizer
  python tools/bench_q8.py --bits 4               # int4, bf16, fp32 + quantizer
  python tools/bench_q8.py --kinds int4,int8,bf16 --hotness 8
  python tools/bench_q8.py --kinds bf16,fp32 --pkg-root <other checkout>

``--bits`` picks the quantized format of the default kinds and of the
quantizer timing; ``--kinds`` may also name ``int4`` and ``int8`` side by
side.  ``--hotness H`` gathers the same ``--nids`` ids as bags of H (sum).
``--pkg-root`` imports the package (and its built extension) from another
checkout, to time the fp32 / bf16 kernels of a different commit in the same
session.
"""
import argparse
import os
import sys
import time

p = argparse.ArgumentParser()
p.add_argument("--bits", type=int, default=8, choices=[4, 8])
p.add_argument("--kinds", default=None,
               help="default: int<bits>,bf16,fp32")
p.add_argument("--pkg-root", default=os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))
p.add_argument("--rows", type=int, default=16_000_000)
p.add_argument("--width", type=int, default=128)
p.add_argument("--nids", type=int, default=213_000)
p.add_argument("--hotness", type=int, default=1)
p.add_argument("--repeats", type=int, default=7)
p.add_argument("--iters", type=int, default=50)
p.add_argument("--no-quantizer", action="store_true")
args = p.parse_args()
sys.path.insert(0, args.pkg_root)

import torch  # noqa: E402
from distributed_embeddings_amd.ops import _backend  # noqa: E402

assert torch.cuda.is_available(), "this benchmark needs the GPU"
ext = _backend.ops()
kinds = (args.kinds or f"int{args.bits},bf16,fp32").split(",")
rows, width, nids = args.rows, args.width, args.nids
nids -= nids % args.hotness
row_bytes = {"int4": width // 2 + 4, "int8": width + 8, "bf16": 2 * width,
             "fp32": 4 * width}
assert all(k in row_bytes for k in kinds), kinds
quantizers = {"int4": getattr(ext, "quantize_rows_q4", None),
              "int8": ext.quantize_rows_q8}
forwards = {"int4": getattr(ext, "csr_lookup_forward_q4", None),
            "int8": ext.csr_lookup_forward_q8}


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


g = torch.Generator(device="cuda").manual_seed(1)
# values in a narrow band per row, as trained embeddings are; built in chunks
# so the fp32 source of a quantized table never exists whole
tables = {}
chunk = 1 << 20
for kind in kinds:
    if kind in quantizers:
        t = torch.empty(rows, row_bytes[kind], dtype=torch.uint8,
                        device="cuda")
    else:
        t = torch.empty(rows, width, device="cuda",
                        dtype=torch.bfloat16 if kind == "bf16" else torch.float32)
    for s in range(0, rows, chunk):
        src = torch.randn(min(chunk, rows - s), width, device="cuda",
                          generator=g)
        if kind in quantizers:
            t[s:s + chunk].copy_(quantizers[kind](src))
        else:
            t[s:s + chunk].copy_(src)
    tables[kind] = t
pools = [torch.randint(0, rows, (nids,), device="cuda", generator=g)
         for _ in range(16)]
splits = torch.arange(nids // args.hotness + 1, device="cuda") * args.hotness
it = [0]


def cold_ids():
    it[0] += 1
    return pools[it[0] % len(pools)]


def lookup(kind):
    if kind in forwards:
        return forwards[kind](tables[kind], cold_ids(), splits, False)
    return ext.csr_lookup_forward(tables[kind], cold_ids(), splits, False)


print(f"pkg {args.pkg_root}: rows {rows} width {width} nids {nids} "
      f"hotness {args.hotness} iters {args.iters}")
rates = {k: [] for k in kinds}
for _ in range(args.repeats):
    for kind in kinds:
        rates[kind].append(nids / timeit(lambda: lookup(kind), args.iters))
for kind in kinds:
    r = sorted(rates[kind])
    med = r[len(r) // 2]
    print(f"{kind:5s} rows/s " + " ".join(f"{x / 1e6:7.1f}M" for x in rates[kind])
          + f" | median {med / 1e6:.1f}M spread {(r[-1] - r[0]) / 1e6:.1f}M"
          f" | {row_bytes[kind]} B/row -> {med * row_bytes[kind] / 1e9:.0f} GB/s")

qkind = f"int{args.bits}"
if qkind in kinds and not args.no_quantizer:
    src = torch.randn(1 << 20, width, device="cuda", generator=g)
    for dt in (torch.float32, torch.bfloat16):
        x = src.to(dt)
        t = [timeit(lambda: quantizers[qkind](x), 50) for _ in range(5)]
        t.sort()
        moved = x.numel() * x.element_size() + x.shape[0] * row_bytes[qkind]
        name = "quantize_rows" + ("_q4" if args.bits == 4 else "")
        print(f"{name} [1M, {width}] {str(dt)[6:]}: median "
              f"{t[2] * 1e6:.1f} us, {x.shape[0] / t[2] / 1e9:.2f} G rows/s, "
              f"{moved / t[2] / 1e9:.0f} GB/s read+written "
              f"(spread {(t[-1] - t[0]) * 1e6:.1f} us)")
