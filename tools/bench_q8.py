"""Cold random gather from int8 row-wise, bf16 and fp32 tables, one-hot.

The shape of bench_cold.py (213k one-hot rows, width 128, 16 id pools so no
call repeats the previous call's rows) on a table large enough to defeat L2
and the Infinity Cache, with the table kinds alternated inside every repeat so
that drift hits all of them alike.  Prints rows/s per repeat, the median, the
spread (max - min) and the table bytes fetched per second.

  python tools/bench_q8.py                        # int8, bf16, fp32 + quantizer
  python tools/bench_q8.py --kinds bf16,fp32 --pkg-root <other checkout>

``--pkg-root`` imports the package (and its built extension) from another
checkout, to time the fp32 / bf16 kernels of a different commit in the same
session.
"""
import argparse
import os
import sys
import time

p = argparse.ArgumentParser()
p.add_argument("--kinds", default="int8,bf16,fp32")
p.add_argument("--pkg-root", default=os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))
p.add_argument("--rows", type=int, default=16_000_000)
p.add_argument("--width", type=int, default=128)
p.add_argument("--nids", type=int, default=213_000)
p.add_argument("--repeats", type=int, default=7)
p.add_argument("--iters", type=int, default=50)
p.add_argument("--no-quantizer", action="store_true")
args = p.parse_args()
sys.path.insert(0, args.pkg_root)

import torch  # noqa: E402
from distributed_embeddings_amd.ops import _backend  # noqa: E402

assert torch.cuda.is_available(), "this benchmark needs the GPU"
ext = _backend.ops()
kinds = args.kinds.split(",")
rows, width, nids = args.rows, args.width, args.nids


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
# so the fp32 source of the int8 table never exists whole
tables, row_bytes = {}, {"int8": width + 8, "bf16": 2 * width, "fp32": 4 * width}
chunk = 1 << 20
for kind in kinds:
    if kind == "int8":
        t = torch.empty(rows, width + 8, dtype=torch.uint8, device="cuda")
    else:
        t = torch.empty(rows, width, device="cuda",
                        dtype=torch.bfloat16 if kind == "bf16" else torch.float32)
    for s in range(0, rows, chunk):
        src = torch.randn(min(chunk, rows - s), width, device="cuda",
                          generator=g)
        if kind == "int8":
            t[s:s + chunk].copy_(ext.quantize_rows_q8(src))
        else:
            t[s:s + chunk].copy_(src)
    tables[kind] = t
pools = [torch.randint(0, rows, (nids,), device="cuda", generator=g)
         for _ in range(16)]
splits = torch.arange(nids + 1, device="cuda")
it = [0]


def cold_ids():
    it[0] += 1
    return pools[it[0] % len(pools)]


def lookup(kind):
    if kind == "int8":
        return ext.csr_lookup_forward_q8(tables[kind], cold_ids(), splits,
                                         False)
    return ext.csr_lookup_forward(tables[kind], cold_ids(), splits, False)


print(f"pkg {args.pkg_root}: rows {rows} width {width} nids {nids} "
      f"iters {args.iters}")
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

if "int8" in kinds and not args.no_quantizer:
    src = torch.randn(1 << 20, width, device="cuda", generator=g)
    for dt in (torch.float32, torch.bfloat16):
        x = src.to(dt)
        t = [timeit(lambda: ext.quantize_rows_q8(x), 50) for _ in range(5)]
        t.sort()
        moved = x.numel() * x.element_size() + x.shape[0] * (width + 8)
        print(f"quantize_rows [1M, {width}] {str(dt)[6:]}: median "
              f"{t[2] * 1e6:.1f} us, {x.shape[0] / t[2] / 1e9:.2f} G rows/s, "
              f"{moved / t[2] / 1e9:.0f} GB/s read+written "
              f"(spread {(t[-1] - t[0]) * 1e6:.1f} us)")
