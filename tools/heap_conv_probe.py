"""Coherent dedispersion of MeerKAT heaps (DSPSR_AMD_RAW_MEERKAT), the shape of `dspsr -F 1024:D` behind the beamformer: 1024 complex
channels, two polarisations, 8-bit; dsp::Convolution with n_fft 1024 and 4096 and about a quarter of it discarded, detected output.
The one-pass kernel reading the heaps itself (csrc/fb_conv1.hip, k_conv1_heaps) against the engine unpacking first
(k_unpack_heaps, then k_conv1 on float rows: FilterbankEngine.setup(fuse_heaps=False)) -- alternating windows of at least a second
in ONE process, HIP events on the launch stream, every shape warmed up, and the spread of the windows of the same code.
  python tools/heap_conv_probe.py [MiB of 8-bit per block] [n_fft,n_fft,...] [windows per route]
Prints, per n_fft and route, the times per block, the bytes per second the traffic model of DESIGN.md gives that time, and the spread."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dspsr_amd  # noqa: E402

NCHAN = 1024


def model_bytes(n_fft, nsamp_step, fused, out_bytes=16):
    """HBM bytes per dual-polarisation input sample of one channel (4 bytes of 8-bit): what each route reads and writes.
    Every part reads its n_fft samples again, nsamp_step of them new: the re-read factor n_fft / nsamp_step.  Both routes write the
    same output (out_bytes per kept sample, one kept per new input sample)."""
    reread = n_fft / nsamp_step
    if fused:
        return 4 * reread + out_bytes
    return 4 + 16 + 16 * reread + out_bytes                    # unpack: read 4, write 16; the float kernel reads 16 per sample of a part


def main():
    mib = float(sys.argv[1]) if len(sys.argv) > 1 else 256.0
    sizes = [int(a) for a in sys.argv[2].split(",")] if len(sys.argv) > 2 else (1024, 4096)
    nwin = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    ctx = dspsr_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    print("build", dspsr_amd.build_id(), "| %d channels x 2 polarisations, blocks of about %g MiB of 8-bit" % (NCHAN, mib))
    scale = float(dspsr_amd.eight_bit_scale())
    for M in sizes:
        nfilt = (M // 8, M // 8)
        step = M - sum(nfilt)
        npart = max(1, int(mib * (1 << 20)) // (NCHAN * 4) // step)
        nsamp = npart * step + sum(nfilt)
        nheap = -(-nsamp // 256)
        raw = torch.randint(-128, 128, (nheap * 2 * NCHAN * 512,), dtype=torch.int8, device="cuda")
        kernel = np.exp(1j * np.random.default_rng(1).uniform(-np.pi, np.pi, NCHAN * M)).astype(np.complex64)
        det = torch.empty((NCHAN, 1, 4 * npart * step), dtype=torch.float32, device="cuda")
        engs = {name: dspsr_amd.FilterbankEngine(ctx).setup(1, M, nfilt[0], nfilt[1], NCHAN, 2, False, kernel, max_parts=min(npart, 256), fuse_heaps=fuse)
                for name, fuse in (("fused", True), ("unpack+float", False))}
        assert all(e.takes_heaps() for e in engs.values())

        def run(eng):
            eng.perform_detect(det, npart, dspsr_amd.COHERENCE, 4, raw=raw, layout=dspsr_amd.RAW_MEERKAT, scale=scale)

        def timed(eng, reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                run(eng)
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / reps
        reps = {}
        for name, eng in engs.items():                          # warm-up (allocations, first launches), then the window length
            run(eng)
            torch.cuda.synchronize()
            reps[name] = max(1, int(1100.0 / timed(eng, 3)) + 1)
        times = {name: [] for name in engs}
        for _ in range(nwin):                                   # alternating windows of >= 1 s
            for name, eng in engs.items():
                times[name].append(timed(eng, reps[name]))
        new_samples = NCHAN * npart * step                      # dual-polarisation samples a block brings
        print("n_fft %d, nfilt %d + %d, %d parts, block %.1f MiB of 8-bit, windows of %s blocks" % (
            M, nfilt[0], nfilt[1], npart, raw.numel() / (1 << 20), "/".join(str(reps[n]) for n in engs)))
        med = {}
        for name in engs:
            t = sorted(times[name])
            med[name] = t[len(t) // 2]
            by = model_bytes(M, step, name == "fused") * new_samples
            print("  %-13s %9.3f ms per block (windows %s), spread %.2f %%, model %.0f MB -> %.2f TB/s, %.0f M dual-pol samples/s" % (
                name, med[name], " ".join("%.3f" % v for v in times[name]), 100.0 * (t[-1] - t[0]) / med[name], by / 1e6,
                by / med[name] / 1e9, new_samples / med[name] / 1e3))
        print("  fused / unpack+float = %.3f" % (med["fused"] / med["unpack+float"]))
        for e in engs.values():
            e.close()
        del raw, det
    ctx.close()


if __name__ == "__main__":
    main()
