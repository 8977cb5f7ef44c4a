"""Clip interpolation over a YUV4MPEG2 stream, through a file or a pipe:

    ffmpeg -i in.mp4 -f yuv4mpegpipe - | python -m vfi_amd.fusion_net.interpolate_stream --input - --output - | ffmpeg -i - out.mp4

The counterpart of interpolate_video.py's PNG loop without a codec on either side of the frame: the host moves a frame's
bytes with one `readinto` and one `write`, and everything between those bytes and the frame's tensors is two HIP launches
(ops.yuv_to_rgb, ops.rgb_to_yuv).

  * a reader thread fills a ring of pinned host frames, a writer thread emits strictly in stream order: original k as its
    own FRAME line and its own bytes from the ring slot (never decoded and re-encoded), interpolated k behind a plain
    `FRAME\\n`, ..., the last original;
  * each source frame is uploaded and decoded ONCE: one launch writes its rgb and its Lab planes into the (6,H,W) Lab
    buffers of both pairs it belongs to; the pair runs through FusionInterpolator.run_prepared;
  * streams and events as in interpolate_video.py: one HIP stream per runner, the next pair waits for the upload / decode
    event only, `record_stream` on what crosses streams;
  * a ring slot goes back to the reader once its H2D copy has landed and its pass-through write is done.  Its role as the
    first frame of the next pair needs nothing more of the slot: that pair reads the device tensors the one decode wrote.

n input frames give 2n - 1 output frames; the output header is the input's with F doubled (unless `keep_rate`).  A stream is
not sharded over GPUs.  H and W must be multiples of 8 (FusionNet's three 2x poolings).

Two options, both off by default, and off is the loop above launch for launch:
  * `--factor 4 | 8`: a pair's factor - 1 frames come from FusionInterpolator.run_recursive on that pair's stream and
    runner, each with its own rgb_to_yuv, D2H copy and event; n frames give factor (n - 1) + 1, F is multiplied by factor;
  * `--scene_threshold T`: one ops.luma_sad per pair on the two frames' device bytes and one ops.frame_pick per encoded
    frame, which on a cut replaces it by the nearer original's bytes.  The statistic and the decision stay on the
    device; the flag comes back with the pair's first frame and is read by the writer thread (`args.scene_cuts`).
"""
import argparse
import os
import queue
import sys
import threading

from . import scene, y4m


def _check_size(fmt):
    if fmt.width % 8 or fmt.height % 8:
        raise ValueError(f"interpolate_stream: frame size {fmt.width}x{fmt.height}: width and height must be multiples of 8 "
                         "(FusionNet pools three times by 2); pad or crop the stream first, e.g. with ffmpeg's pad filter")


def interpolate_stream(args, src, dst, runners=None, frames_in_flight=2):
    """Interpolates every consecutive pair of the Y4M stream `src` (binary, readable) into `dst` (binary, writable).
    args: gpu_id, matrix ('bt709' | 'bt601'), range ('limited' | 'full'), keep_rate, factor (2 | 4 | 8, default 2),
    scene_threshold (percent, default None = off), and the model fields of build_models when `runners` is None.
    Returns the number of interpolated frames; `args.truncated` tells whether the input stopped inside a frame (the
    complete frames are still finished and flushed), `args.scene_cuts` lists the source pairs flagged as cuts."""
    factor, threshold = getattr(args, "factor", 2), getattr(args, "scene_threshold", None)
    if factor not in (2, 4, 8):
        raise ValueError(f"interpolate_stream: factor must be 2, 4 or 8, got {factor!r}")
    fmt = y4m.read_header(src, getattr(args, "matrix", "bt709"), getattr(args, "range", "limited"))
    _check_size(fmt)                                       # before the first launch, before a byte is written
    cut_sad = None if threshold is None else scene.min_sad(threshold, fmt.width * fmt.height)
    import torch
    from .. import ops
    from .interpolate_twoframe import FusionInterpolator, build_models
    device = torch.device("cuda:{}".format(args.gpu_id))
    torch.cuda.set_device(device)
    if runners is None:
        adacof, fusion = build_models(args, device)
        pn = getattr(args, "phase_net_checkpoint", "./src/phase_net/phase_net.pt")
        state = torch.load(pn, map_location="cpu") if pn and os.path.exists(pn) else None
        runners = [FusionInterpolator(adacof, fusion, state, device) for _ in range(max(1, frames_in_flight))]
    rate = fmt.rate if getattr(args, "keep_rate", False) or fmt.rate is None else (fmt.rate[0] * factor, fmt.rate[1])
    y4m.write_header(dst, fmt, rate)

    h, w, nbytes = fmt.height, fmt.width, fmt.frame_bytes
    n_in, n_out = 2 * max(1, frames_in_flight) + 2, (max(1, frames_in_flight) + 1) * (factor - 1)
    ring = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(n_in)]
    out_ring = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(n_out)]
    ring_np, out_np = [t.numpy() for t in ring], [t.numpy() for t in out_ring]
    cuts = []                                              # pairs flagged on the device, appended by the writer in order
    if cut_sad is not None:                                # a pair's flag lands next to its first frame's bytes
        out_flag = torch.zeros(n_out, dtype=torch.int32, pin_memory=True)
        out_flag_np = out_flag.numpy()
    free, out_free, filled, to_write = queue.Queue(), queue.Queue(), queue.Queue(), queue.Queue()
    for i in range(n_in):
        free.put(i)
    for i in range(n_out):
        out_free.put(i)
    errors = []
    stop = threading.Event()                               # set on a failure anywhere: the reader stops taking slots

    def reader():
        try:
            while not stop.is_set():
                slot = free.get()
                if slot is None:
                    break
                line = y4m.read_frame_into(src, ring_np[slot], fmt)
                if line is None:
                    break
                filled.put((slot, line))
        except BaseException as e:                         # noqa: BLE001 (re-raised by the caller's thread below)
            errors.append(e)
        finally:
            filled.put(None)

    def writer():
        failed = False
        while True:
            item = to_write.get()
            if item is None:
                break
            kind, slot, line, event, flagged = item
            try:
                if kind == "original":                     # the slot's own bytes; then wait for its H2D copy and hand it back
                    if not failed:
                        y4m.write_frame(dst, line, ring_np[slot])
                    event.synchronize()
                else:                                      # the D2H copy of this frame has landed in its pinned buffer
                    event.synchronize()
                    if flagged is not None and out_flag_np[slot]:      # (the pair's flag came with its first frame)
                        cuts.append(flagged)
                    if not failed:
                        y4m.write_frame(dst, line, out_np[slot])
            except BaseException as e:                     # noqa: BLE001 (keep draining: the other threads wait on the slots)
                if not failed:
                    errors.append(e)
                failed = True
                stop.set()
            (free if kind == "original" else out_free).put(slot)

    threads = [threading.Thread(target=reader, name="y4m-reader", daemon=True),
               threading.Thread(target=writer, name="y4m-writer", daemon=True)]
    for t in threads:
        t.start()
    streams = [torch.cuda.Stream(device=device) for _ in runners]
    # of frame k - 1: (rgb, lab12 with its first half filled, decode event, its bytes on the device, the SAD word of the pair
    # it closed); the last two are read only with a scene threshold
    prev = None
    k = written = 0
    try:
        while True:
            item = filled.get()
            if item is None or errors:
                break
            slot, line = item
            pair = max(k - 1, 0)                           # frame k closes pair k - 1 and is uploaded on that pair's stream
            s, runner = streams[pair % len(runners)], runners[pair % len(runners)]
            oslots = [out_free.get() for _ in range(factor - 1)] if prev is not None else []
            done, sad = [], None
            with torch.cuda.stream(s):
                frame = torch.empty(nbytes, dtype=torch.uint8, device=device)
                frame.copy_(ring[slot], non_blocking=True)
                h2d = torch.cuda.Event()
                h2d.record(s)
                rgb = torch.empty((3, h, w), dtype=torch.float32, device=device)
                lab12 = torch.empty((6, h, w), dtype=torch.float32, device=device)   # of pair k: this frame is its first
                if prev is not None:                       # uploaded and decoded on another stream
                    s.wait_event(prev[2])
                    prev[0].record_stream(s)
                    prev[1].record_stream(s)
                ops.yuv_to_rgb(frame, h, w, fmt, rgb=rgb, lab=(lab12[:3], prev[1][3:] if prev is not None else None))
                if cut_sad is not None and prev is not None:   # both frames' bytes are on the device; before `up`, so that
                    prev[3].record_stream(s)                   # the next pair's wait covers this word too
                    sad = ops.luma_sad(prev[3], frame, h * w)
                up = torch.cuda.Event()
                up.record(s)                               # the next pair waits for this, not for this pair's compute
                if prev is not None:
                    finals = runner.run_recursive(prev[0], rgb, prev[1], factor)
                    for j, (final, oslot) in enumerate(zip(finals, oslots), 1):      # the frame at t = j / factor
                        enc = ops.rgb_to_yuv(final, fmt)
                        if sad is not None:                # on a cut: the nearer original's bytes (the first at t = 1/2)
                            if prev[4] is not None:
                                prev[4].record_stream(s)
                            flag = torch.empty(1, dtype=torch.int32, device=device) if j == 1 else None
                            ops.frame_pick(enc, prev[3] if 2 * j <= factor else frame, sad, prev[4], cut_sad, cut=flag)
                            if flag is not None:
                                out_flag[oslot:oslot + 1].copy_(flag, non_blocking=True)
                        out_ring[oslot].copy_(enc, non_blocking=True)
                        d2h = torch.cuda.Event()
                        d2h.record(s)
                        done.append(d2h)
            for j, (oslot, d2h) in enumerate(zip(oslots, done)):
                to_write.put(("interpolated", oslot, b"FRAME\n", d2h, pair if sad is not None and j == 0 else None))
                written += 1
            to_write.put(("original", slot, line, h2d, None))
            prev = (rgb, lab12, up, frame, sad)
            k += 1
    except BaseException as e:                             # noqa: BLE001
        errors.insert(0, e)
    finally:
        stop.set()
        to_write.put(None)
        threads[1].join()
        free.put(None)                                     # a reader waiting for a slot ends; one inside read() ends with its stream
        torch.cuda.synchronize(device)
    if errors:
        raise errors[0]
    threads[0].join()
    dst.flush()
    args.truncated = bool(fmt.truncated)
    args.scene_cuts = cuts
    return written


parser = argparse.ArgumentParser(description="Video interpolation over a YUV4MPEG2 stream")
parser.add_argument("--input", type=str, default="-", help="a .y4m file, or - for stdin")
parser.add_argument("--output", type=str, default="-", help="a .y4m file, or - for stdout")
parser.add_argument("--gpu_id", type=int, default=0)
parser.add_argument("--adacof_model", type=str, default="vfi_amd.fusion_net.fusion_adacofnet")
parser.add_argument("--adacof_checkpoint", type=str, default="./src/adacof/checkpoint/kernelsize_5/ckpt.pth")
parser.add_argument("--adacof_config", type=str, default="./src/adacof/checkpoint/kernelsize_5/config.txt")
parser.add_argument("--adacof_kernel_size", type=int, default=5)
parser.add_argument("--adacof_dilation", type=int, default=1)
parser.add_argument("--checkpoint", type=str, default="./src/fusion_net/fusion_net1.pt")
parser.add_argument("--phase_net_checkpoint", type=str, default="./src/phase_net/phase_net.pt")
parser.add_argument("--model", type=int, default=1)
parser.add_argument("--matrix", type=str, choices=sorted(y4m.MATRICES), default="bt709")
parser.add_argument("--range", type=str, choices=sorted(y4m.RANGES), default="limited",
                    help="the header's XCOLORRANGE token wins over this")
parser.add_argument("--keep_rate", action="store_true", help="leave the header's F token alone (slow motion)")
parser.add_argument("--frames_in_flight", type=int, default=2)
parser.add_argument("--factor", type=int, choices=(2, 4, 8), default=2,
                    help="frame-rate multiple: 4 and 8 interpolate between an original and an interpolated frame")
parser.add_argument("--scene_threshold", type=float, default=None,
                    help="off by default.  Percent of the luma range: a pair whose mean absolute luma difference m gives "
                         "min(m, |m - m of the previous pair|) >= this is a scene cut, and the nearer original is repeated "
                         "in place of its interpolated frames.  ffmpeg's scdet filter documents this rule with a default of "
                         "10, a starting point; no footage was used to tune anything here")


def main(argv=None):
    args = parser.parse_args(argv)
    src = dst = None
    try:
        if args.output == "-":
            # the data owns the process's stdout; everything anything prints from here on (progress, warnings, the model
            # builders, native code) goes to stderr
            sys.stdout.flush()
            dst = os.fdopen(os.dup(1), "wb")
            os.dup2(2, 1)
            sys.stdout = sys.stderr
        else:
            dst = open(args.output, "wb")
        src = os.fdopen(os.dup(0), "rb") if args.input == "-" else open(args.input, "rb")
        done = interpolate_stream(args, src, dst, frames_in_flight=args.frames_in_flight)
        dst.flush()
        cuts = "" if args.scene_threshold is None else f", {len(args.scene_cuts)} scene cuts"
        print(f"interpolate_stream: {done} interpolated frames{cuts}", file=sys.stderr)
        if args.truncated:
            print("interpolate_stream: warning: the input stopped inside a frame; the complete frames were written",
                  file=sys.stderr)
            return 1
        return 0
    finally:
        for f in (dst, src):
            if f is not None:
                f.close()


if __name__ == "__main__":
    sys.exit(main())
