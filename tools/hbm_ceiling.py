"""What a plain streaming kernel reaches on this box (reference point for the element-wise / 1x1 kernels' HBM fractions):
torch's copy_, add(out=) and a read-only sum over tensors far larger than the 256 MB of Infinity Cache.  ``ceiling(dtype, leg)`` is
one figure in TB/s for other tools (tools/detector_trunk_bench.py); run as a script it prints all six."""
import torch

N = 1 << 29   # 512 Mi elements
LEGS = {"copy": ("copy (1 read + 1 write)", 2), "add": ("add  (2 reads + 1 write)", 3), "sum": ("sum  (1 read)", 1)}


def measure(dt, dev):
    """{leg: (microseconds, TB/s)} for tensors of N elements of dtype dt."""
    x = torch.empty(N, dtype=dt, device=dev).normal_()
    y = torch.empty_like(x).normal_()
    z = torch.empty_like(x)
    nb = x.numel() * x.element_size()
    out = {}
    for leg, fn in (("copy", lambda: z.copy_(x)), ("add", lambda: torch.add(x, y, out=z)), ("sum", lambda: x.sum())):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 10
        out[leg] = (ms * 1e3, LEGS[leg][1] * nb / ms / 1e9)
    return out


def ceiling(dt=torch.float32, leg="copy", dev="cuda") -> float:
    """TB/s of one leg."""
    return measure(dt, torch.device(dev))[leg][1]


if __name__ == "__main__":
    for dt in (torch.float16, torch.float32):
        nb = N * torch.empty(0, dtype=dt).element_size()
        for leg, (us, tbps) in measure(dt, torch.device("cuda")).items():
            print(f"{str(dt):14s} {LEGS[leg][0]:26s} {nb / 2**20:6.0f} MiB per tensor: {us:8.1f} us  {tbps:7.2f} TB/s")
