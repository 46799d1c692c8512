"""Frame files decoded on the GPU, bit-identical to PIL: the decode step of the reference's input chains.
  JPEG (csrc/jpeg.hip, csrc/jpeg_core.h): the student-side reader's PIL.Image.open(f).load() (video_reader.py:334-343)
  PNG  (csrc/png.hip, csrc/png_core.h): the teacher-side readers' Image.open(path).convert("RGB") (AuxDataset.py:129-136,
       teacher/code/video_reader.py:190-199)
A FormatPlan is the host half of a batch of one format (JpegPlan, PngPlan: siblings that differ in their format facts only), an ImagePlan
sorts a batch of either format into the two.  ops.py does not import this module."""
import ctypes
import itertools

import torch

from ._lib import lib
from .ops import _p, device_index

SUPPORTED, UNSUPPORTED, MALFORMED = 0, 1, 2      # a planner's verdict on an image (both C planners: PST_OK .. in csrc/png_core.h)
JPEG_DEVICE_ERRORS = {1: "bad Huffman code", 2: "coefficient index past 63", 3: "entropy-coded data ends early",
                      4: "restart marker out of sequence", 5: "data left over at the end of the scan",
                      6: "entropy-coded data does not fit the decoder's window"}
PNG_DEVICE_ERRORS = {1: "bad deflate block type", 2: "stored block LEN / NLEN mismatch", 3: "bad code lengths",
                     4: "invalid length or distance symbol", 5: "distance too far back", 6: "more data than the image holds",
                     7: "data ends early", 8: "filter type above 4", 9: "Adler-32 mismatch",
                     10: "compressed data does not fit the decoder's window"}
_SCRATCH = {}      # (format, device index, stream) -> {"in", ...}: a plan's device buffers, grown on demand, reused in stream order
_NOT_UPLOADED = "not uploaded"      # a pinned slot's "event" from PinnedRing.get() until its plan's decode() has queued the H2D copy


def _align(n, a=256):
    return (int(n) + a - 1) // a * a


def _scratch(key, need, dev):
    """the device buffers of `key`: need = {name: (elements needed, dtype)}; "in" holds the uploaded plan, the others what the launches
    pass between them.  All are reallocated together (a quarter above the largest need so far) when any one is too small."""
    sc = _SCRATCH.get(key)
    if sc is None or any(sc[k].numel() < n for k, (n, _) in need.items()):
        old = {k: t.numel() for k, t in sc.items()} if sc else {}
        sc = _SCRATCH[key] = {k: torch.empty(_align(max(n, old.get(k, 0)) * 5 // 4, 1 << 20) if k == "in" else _align(max(n, old.get(k, 0), 64) * 5 // 4),
                                             dtype=dt, device=dev) for k, (n, dt) in need.items()}
    return sc


def _words(status):
    return status.tolist() if torch.is_tensor(status) else list(status)


def _stats(rec, reset):
    out = dict(rec)
    if reset:
        rec.update(dict.fromkeys(rec, 0))
    return out


def _out(who, shapes, total, out, device):
    """validate `out` (any contiguous uint8 device tensor of `total` bytes) or allocate it -> (out, its flat view, the device)"""
    dev = torch.device(device) if device is not None else (out.device if out is not None else torch.device("cuda", torch.cuda.current_device()))
    if out is None:
        out = torch.empty((len(shapes),) + shapes[0] + (3,) if len(set(shapes)) == 1 else (total,), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or not out.is_contiguous() or not out.is_cuda or out.numel() != total:
        raise RuntimeError("%s_decode: `out` must be a contiguous uint8 device tensor of %d bytes" % (who, total))
    return out, out.view(-1), dev


def _frames(out, flat, shapes, offs):
    """what decode() returns of its output: `out` itself if it is 4-D, a list of [H, W, 3] views (image i at offs[i]) if the sizes differ,
    else [n, H, W, 3]"""
    if out.dim() == 4:
        return out
    if len(set(shapes)) != 1:
        return [flat[o:o + h * w * 3].view(h, w, 3) for o, (h, w) in zip(offs, shapes)]
    return flat.view((len(shapes),) + shapes[0] + (3,))


def split_videos(frames, L):
    """decode()'s frames (a [F, H, W, 3] tensor, or a list of F [H, W, 3] tensors), video-major -> list of F // L videos [L, H, W, 3]:
    views of the tensor, stacked copies of a list's frames"""
    cut = (lambda v: v) if torch.is_tensor(frames) else torch.stack
    return [cut(frames[i * L:(i + 1) * L]) for i in range(len(frames) // L)]


class PinnedRing:
    """a ring of pinned host buffers for the plans (pinning a fresh buffer per episode costs milliseconds of hipHostMalloc).
    A slot's "event" says what may be done with its buffer:
      None            nothing reads it: reused as it is
      an event        decode() recorded it after the H2D copy that reads the buffer: reused once it has passed
      _NOT_UPLOADED   handed to a plan whose decode() has not run yet (a prefetch thread builds plans ahead of the consumer): no event
                      to wait for, so the buffer stays with that plan and a fresh one takes the slot.  A loader sizes the ring so that
                      this does not happen in its steady state; when it does, it costs one allocation, never a frame.
    An ImagePlan draws the buffers of its two formats from two lanes (lane()), each a ring of this size: an episode then takes one slot
    of a lane whether it holds one format or both, and the ring wraps after the same number of episodes.  pin=False: pageable buffers
    (a host without a GPU)."""

    def __init__(self, n=6, pin=True):
        self.slots = [None] * max(2, int(n))
        self.i = 0
        self.pin = pin
        self._lanes = {}

    def lane(self, key):
        """the ring of the same size that serves `key` alone"""
        if key not in self._lanes:
            self._lanes[key] = PinnedRing(len(self.slots), self.pin)
        return self._lanes[key]

    def get(self, nbytes):
        k = self.i % len(self.slots)
        self.i += 1
        s = self.slots[k]
        if s is not None and s["event"] is _NOT_UPLOADED:
            s = None
        elif s is not None and s["event"] is not None:
            s["event"].synchronize()
        if s is None or s["buf"].numel() < nbytes:
            buf = torch.empty(_align(nbytes * 5 // 4, 1 << 20), dtype=torch.uint8)
            s = self.slots[k] = {"buf": buf.pin_memory() if self.pin else buf}
        s["event"] = _NOT_UPLOADED
        return s


def _pil_decode(data, name, convert_rgb=False, label="JPEG"):
    """the reference's own decoder for the images the plan marks unsupported (progressive, arithmetic, grayscale, interlaced, 16-bit,
    ...).  convert_rgb: the teacher-side readers' Image.open(path).convert("RGB") (AuxDataset.py:129-136); without it a mode other than
    RGB raises, as the student-side reader (video_reader.py:334-343) hands the frame transform whatever mode the file has"""
    import io
    import numpy as np
    from PIL import Image
    try:
        with Image.open(io.BytesIO(data)) as im:
            im.load()
            if im.mode != "RGB":
                if not convert_rgb:
                    raise ValueError("%s %s: PIL decodes it as mode %s, the frame transform takes RGB" % (label, name, im.mode))
                return np.array(im.convert("RGB"))
            return np.array(im)
    except (OSError, SyntaxError) as e:      # damage in a file the plan leaves to PIL: named like every other damaged image
        raise ValueError("%s %s is malformed: PIL refuses it: %s" % (label, name, e)) from e


class _Batch:
    """what the loaders use of a plan, from its walk in batch order: _each() -> (the FormatPlan that owns the image, its index there)"""

    def shapes(self):
        return [p.shape(i) for p, i in self._each()]

    def verdicts(self):
        """[(verdict, reason text)] per image"""
        return [(int(p.info[i, 0]), p._reason(i)) for p, i in self._each()]

    def check(self):
        """ValueError naming the first image whose header or table its plan found malformed"""
        for p, i in self._each():
            e = p.malformed(i)
            if e is not None:
                raise e

    def raise_on_status(self, status):
        """ValueError naming the first image the GPU decoder stopped (status: the host copy of decode()'s status words)"""
        for (p, i), s in zip(self._each(), _words(status)):
            if s:
                raise p.stopped(i, s)


class FormatPlan(_Batch):
    """The host half of a batch decode of one format (lmkd_<format>_plan): the images' bytes, their descriptors and the table pool in ONE
    host buffer laid out [descriptors | data | pool] (pinned when a GPU is present: one H2D copy of the used prefix), the verdict per
    image, and the PIL decode of the images the plan marks unsupported (done here, on the thread that builds the plan - a loader's
    prefetch thread).  A format supplies its C infix, label, device error table and stats record (_C, _LABEL, _ERRORS, _STATS), its
    device buffers (_need) and its launches (_launch); _need also sizes the buffers of the host twin (_decode_host).

    blobs: list of bytes / uint8 tensors, or one packed uint8 tensor with `offsets` (n + 1 byte offsets).  names: optional per-image names
    for the error messages (a loader passes the frame files).  fallback=False skips the PIL decode (the plan's verdicts alone).
    convert_rgb: the PIL fallback returns im.convert("RGB") instead of raising on another mode.  index: the images' positions in a
    larger batch (ImagePlan), used in place of their own in the messages."""

    def __init__(self, blobs, offsets=None, names=None, ring=None, pin=None, fallback=True, convert_rgb=False, index=None):
        import numpy as np
        if offsets is not None:
            packed = blobs.reshape(-1) if torch.is_tensor(blobs) else torch.frombuffer(bytearray(blobs), dtype=torch.uint8)
            offs = [int(o) for o in offsets]
            blobs = [packed[offs[i]:offs[i + 1]].numpy() for i in range(len(offs) - 1)]
        else:
            blobs = [b.cpu().reshape(-1).numpy() if torch.is_tensor(b) else np.frombuffer(b, dtype=np.uint8) for b in blobs]
        n = len(blobs)
        if n == 0:
            raise ValueError("%s_decode: no images" % self._C)
        self.n, self.names, self.index = n, names, index
        sizes = [len(b) for b in blobs]
        dbytes = lib().value("lmkd_%s_desc_bytes" % self._C)
        self.data_off = _align(n * dbytes)
        self.pool_off = _align(self.data_off + sum(sizes))
        pool_cap = lib().value("lmkd_%s_pool_bytes" % self._C, n)
        need = self.pool_off + pool_cap
        pin = torch.cuda.is_available() if pin is None else pin
        if ring is not None and pin:
            self.slot = ring.get(need)
        else:
            buf = torch.empty(need, dtype=torch.uint8)
            self.slot = {"buf": buf.pin_memory() if pin else buf, "event": None}
        self.buf = self.slot["buf"]
        arr = self.buf.numpy()
        offs = [0]
        for b in blobs:
            p = self.data_off + offs[-1]
            arr[p:p + len(b)] = b
            offs.append(offs[-1] + len(b))
        self.offsets = np.asarray(offs, dtype=np.int64)
        self.info = np.zeros((n, 5), dtype=np.int64)
        self.totals = np.zeros(5, dtype=np.int64)
        base = self.buf.data_ptr()
        lib().call("lmkd_%s_plan" % self._C, ctypes.c_void_p(base + self.data_off), ctypes.c_void_p(self.offsets.ctypes.data), n, ctypes.c_void_p(base),
                   ctypes.c_void_p(base + self.pool_off), pool_cap, ctypes.c_void_p(self.info.ctypes.data), ctypes.c_void_p(self.totals.ctypes.data))
        self.nbytes = self.pool_off + int(self.totals[0])          # what the device needs
        self.fallback = {}
        if fallback and not (self.info[:, 0] == MALFORMED).any():
            for i in np.nonzero(self.info[:, 0] == UNSUPPORTED)[0]:
                i = int(i)
                img = _pil_decode(bytes(arr[self.data_off + offs[i]:self.data_off + offs[i + 1]]), self.name(i), convert_rgb, self._LABEL)
                if img.shape[:2] != self.shape(i):
                    raise ValueError("%s %s: PIL decodes %s, the header says %s" % (self._LABEL, self.name(i), img.shape[:2], self.shape(i)))
                t = torch.from_numpy(img)
                self.fallback[i] = t.pin_memory() if pin else t

    def name(self, i):
        return "image %d%s" % (i if self.index is None else self.index[i], " (%s)" % self.names[i] if self.names is not None else "")

    def _reason(self, i):
        return lib().value("lmkd_%s_reason" % self._C, int(self.info[i, 1])).decode()

    def _each(self):
        return ((self, i) for i in range(self.n))

    def shape(self, i):
        return int(self.info[i, 2]), int(self.info[i, 3])

    def malformed(self, i):
        """the ValueError naming image i if the plan found its header or table malformed, else None"""
        if self.info[i, 0] == MALFORMED:
            return ValueError("%s %s is malformed: %s" % (self._LABEL, self.name(i), self._reason(i)))

    def stopped(self, i, s):
        """the ValueError naming image i, which the GPU decoder stopped with status word s"""
        return ValueError("%s %s is malformed: %s" % (self._LABEL, self.name(i), self._ERRORS.get(int(s), "error %d" % s)))

    def check(self):      # (decode() runs check() and shapes() in front of its first launch: one pass over the table each, not a walk)
        if (self.info[:, 0] == MALFORMED).any():
            super().check()

    def shapes(self):
        return list(map(tuple, self.info[:, 2:4].tolist()))

    def release(self):
        """this plan will not be decoded: its ring slot may be reused"""
        if self.slot["event"] is _NOT_UPLOADED:
            self.slot["event"] = None

    def _head(self, buf):
        """the leading arguments of the decode entry points: the data, descriptors and pool of the plan as laid out in `buf`, the count"""
        base = buf.data_ptr()
        return ctypes.c_void_p(base + self.data_off), ctypes.c_void_p(base), ctypes.c_void_p(base + self.pool_off), self.n

    def decode(self, out=None, check=True, device=None):
        """the decode launches on the current stream (+ the H2D copy, + the copies of the PIL-decoded fallback images) -> (frames,
        status): frames = uint8 [F, H, W, 3] when every image has the same size (or `out`, any contiguous uint8 tensor of the total size),
        else a list of [H, W, 3] views; status = int32 device tensor, 0 or the error that stopped the image.  check: read the status words
        (a synchronisation) and raise ValueError for a malformed image; a streamed loader passes False and reads them later."""
        self.check()
        shapes = self.shapes()
        out, flat, dev = _out(self._C, shapes, int(self.totals[2]), out, device)
        stream = torch.cuda.current_stream(dev)
        sc = _scratch((self._C, device_index(dev), stream.cuda_stream), self._need(), dev)
        sc["in"][:self.nbytes].copy_(self.buf[:self.nbytes], non_blocking=True)
        ev = None                                                   # (a pageable buffer has been read when copy_ returns)
        if self.buf.is_pinned():
            ev = torch.cuda.Event()
            ev.record(stream)
        self.slot["event"] = ev                                     # the host buffer may be reused once the copy has run
        status = torch.empty(self.n, dtype=torch.int32, device=dev)
        self._launch(self._head(sc["in"]), sc, flat, status, ctypes.c_void_p(stream.cuda_stream))
        for i, img in self.fallback.items():
            o = int(self.info[i, 4])
            flat[o:o + img.numel()].copy_(img.view(-1), non_blocking=True)
        self._STATS["images"] += self.n
        self._STATS["fallback"] += len(self.fallback)
        self._STATS["gpu"] += self.n - len(self.fallback)
        if check:
            self.raise_on_status(status.cpu())
        return _frames(out, flat, shapes, self.info[:, 4].tolist()), status


class JpegPlan(FormatPlan):
    """lmkd_jpeg_plan / lmkd_jpeg_decode: three launches (entropy pass -> "coef", dequantisation + IDCT -> "planes", upsampling + YCbCr to RGB -> frames)"""
    _C, _LABEL, _ERRORS, _STATS = "jpeg", "JPEG", JPEG_DEVICE_ERRORS, {"images": 0, "gpu": 0, "fallback": 0}

    def _need(self):
        blocks = int(self.totals[1])
        return {"in": (self.nbytes, torch.uint8), "coef": (blocks * 64, torch.int16), "planes": (blocks * 64, torch.uint8)}

    def _launch(self, head, sc, flat, status, stream):
        lib().call("lmkd_jpeg_decode", *head, _p(sc["coef"]), _p(sc["planes"]), _p(flat), _p(status), int(self.totals[3]), int(self.totals[4]), stream)


class PngPlan(FormatPlan):
    """lmkd_png_plan / lmkd_png_decode: two launches (inflate -> the scanlines in "scr", unfilter + expansion to RGB -> frames); the pool
    holds the palettes.  The plan moves the IDAT payloads of a supported image together inside this buffer's copy of the file; the
    caller's bytes are not touched."""
    _C, _LABEL, _ERRORS, _STATS = "png", "PNG", PNG_DEVICE_ERRORS, {"images": 0, "gpu": 0, "fallback": 0}

    def _need(self):
        return {"in": (self.nbytes, torch.uint8), "scr": (int(self.totals[1]), torch.uint8)}

    def _launch(self, head, sc, flat, status, stream):
        trailer = torch.empty(self.n, dtype=torch.int32, device=status.device)
        lib().call("lmkd_png_decode", *head, _p(sc["scr"]), _p(flat), _p(status), _p(trailer), int(self.totals[4]), stream)


def jpeg_stats(reset=False):
    """images handled by jpeg_decode so far: {"images", "gpu", "fallback"} (fallback: decoded on the host with PIL because the plan
    marked them unsupported)"""
    return _stats(JpegPlan._STATS, reset)


def png_stats(reset=False):
    """the same record of png_decode"""
    return _stats(PngPlan._STATS, reset)


def jpeg_decode(blobs, out=None, offsets=None, names=None, check=True):
    """decode a batch of JPEG images on the GPU (current stream) -> (frames, status): see FormatPlan.decode.  blobs: list of bytes / uint8
    tensors, one packed uint8 tensor with `offsets`, or a JpegPlan built beforehand (a loader's prefetch thread).  Images the plan marks
    unsupported are decoded with PIL (counted in jpeg_stats()); a malformed image raises ValueError naming its index."""
    plan = blobs if isinstance(blobs, JpegPlan) else JpegPlan(blobs, offsets=offsets, names=names)
    return plan.decode(out=out, check=check)


def png_decode(blobs, out=None, offsets=None, names=None, check=True):
    """the counterpart of jpeg_decode for PNG images (a PngPlan; png_stats())"""
    plan = blobs if isinstance(blobs, PngPlan) else PngPlan(blobs, offsets=offsets, names=names)
    return plan.decode(out=out, check=check)


def _decode_host(plan, entry):
    """a host twin (lmkd_<format>_decode_host*): the device routines run on the CPU, the tests' reference -> (list of uint8 [H, W, 3] numpy
    arrays, None for images the plan does not decode on the GPU; the plan; status per image).  A malformed image keeps its verdict in
    the plan."""
    import numpy as np
    P = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    # the buffers between the passes, sized like the device's (torch aligns its host buffers to 64 bytes)
    mid = [torch.zeros(max(64, n), dtype=dt).numpy() for k, (n, dt) in plan._need().items() if k != "in"]
    out = np.zeros(max(1, int(plan.totals[2])), dtype=np.uint8)
    status = np.zeros(plan.n, dtype=np.int32)
    lib().call(entry, *plan._head(plan.buf), *map(P, mid), P(out), P(status))
    imgs = []
    for i, (h, w) in enumerate(plan.shapes()):
        o = int(plan.info[i, 4])
        imgs.append(out[o:o + h * w * 3].reshape(h, w, 3).copy() if plan.info[i, 0] == SUPPORTED else None)
    return imgs, plan, status


def jpeg_decode_host(blobs, windowed=False, fallback=True):
    """_decode_host of lmkd_jpeg_decode_host.  windowed: lmkd_jpeg_decode_host_windowed, the entropy launch's own program (window, refill,
    staging, flush) with the wave's lanes run in turn.  fallback=False builds the plan without the PIL decode of the unsupported images
    (a batch of damaged files)."""
    return _decode_host(JpegPlan(blobs, pin=False, fallback=fallback), "lmkd_jpeg_decode_host_windowed" if windowed else "lmkd_jpeg_decode_host")


def png_decode_host(blobs):
    """_decode_host of lmkd_png_decode_host"""
    return _decode_host(PngPlan(blobs, pin=False, fallback=False), "lmkd_png_decode_host")


def _image_format(blob, label):
    head = bytes(blob[:4].tolist()) if torch.is_tensor(blob) else bytes(blob[:4])
    if head[:2] == b"\xff\xd8":
        return "jpeg"
    if head == b"\x89PNG":
        return "png"
    raise ValueError("%s: neither a JPEG nor a PNG signature (first bytes %s)" % (label, head.hex() or "none"))


class ImagePlan(_Batch):
    """A batch of frames of either format: the images are sorted by file signature into a JpegPlan and a PngPlan, and the pair answers
    what trainloop.StreamedEpisodes and the loaders use of a plan: n, shapes(), check(), decode(out=, check=, device=) -> (frames,
    status), raise_on_status(words), verdicts().  A batch of one format decodes straight into `out`; a mixed one decodes each format
    into a buffer of its own and places the frames with one device copy per format.  Any other signature raises ValueError naming the
    file.  convert_rgb: the PIL fallback of both formats returns im.convert("RGB") (the teacher-side readers); without it a frame PIL
    does not decode as RGB raises (the student-side reader)."""

    def __init__(self, blobs, names=None, ring=None, pin=None, fallback=True, convert_rgb=False):
        blobs = list(blobs)
        if not blobs:
            raise ValueError("image_decode: no images")
        self.n, self.names = len(blobs), names
        label = lambda i: "image %d%s" % (i, " (%s)" % names[i] if names is not None else "")      # noqa: E731
        fmt = [_image_format(b, label(i)) for i, b in enumerate(blobs)]
        self.plans = []                     # (plan, positions of its images in the batch)
        for cls in (JpegPlan, PngPlan):
            idx = [i for i, g in enumerate(fmt) if g == cls._C]
            if idx:
                sub = [names[i] for i in idx] if names is not None else None
                self.plans.append((cls([blobs[i] for i in idx], names=sub, ring=ring.lane(cls._C) if ring is not None else None, pin=pin, fallback=fallback,
                                       convert_rgb=convert_rgb, index=idx if len(idx) != self.n else None), idx))
        self._where = [None] * self.n       # batch position -> (owning plan, the image's index there)
        for plan, idx in self.plans:
            for li, i in enumerate(idx):
                self._where[i] = (plan, li)

    def release(self):
        """this batch will not be decoded: its ring slots may be reused"""
        for plan, _ in self.plans:
            plan.release()

    def fallback_images(self):
        """{position in the batch: uint8 [H, W, 3] tensor} of the images PIL decoded on the host"""
        return {idx[li]: img for plan, idx in self.plans for li, img in plan.fallback.items()}

    def _each(self):
        return self._where

    def check(self):
        if any((plan.info[:, 0] == MALFORMED).any() for plan, _ in self.plans):
            super().check()

    def shape(self, i):
        plan, li = self._where[i]
        return plan.shape(li)

    def decode(self, out=None, check=True, device=None):
        self.check()
        if len(self.plans) == 1:
            return self.plans[0][0].decode(out=out, check=check, device=device)
        shapes = self.shapes()
        sizes = [h * w * 3 for h, w in shapes]
        out, flat, dev = _out("image", shapes, sum(sizes), out, device)
        uniform = len(set(shapes)) == 1
        status = torch.zeros(self.n, dtype=torch.int32, device=dev)
        offs = list(itertools.accumulate(sizes, initial=0))
        for plan, idx in self.plans:
            part = torch.empty(sum(sizes[i] for i in idx), dtype=torch.uint8, device=dev)
            _, st = plan.decode(out=part, check=False, device=dev)
            where = torch.tensor(idx, dtype=torch.int64, device=dev)
            status.index_copy_(0, where, st)
            if uniform:
                flat.view(self.n, -1).index_copy_(0, where, part.view(len(idx), -1))
            else:
                o = 0
                for i in idx:
                    flat[offs[i]:offs[i + 1]].copy_(part[o:o + sizes[i]])
                    o += sizes[i]
        if check:
            self.raise_on_status(status.cpu())
        return _frames(out, flat, shapes, offs), status


def image_decode(blobs, out=None, names=None, check=True, convert_rgb=False):
    """decode a batch of JPEG and / or PNG images on the GPU (current stream) -> (frames, status): see ImagePlan"""
    plan = blobs if isinstance(blobs, ImagePlan) else ImagePlan(blobs, names=names, convert_rgb=convert_rgb)
    return plan.decode(out=out, check=check)

