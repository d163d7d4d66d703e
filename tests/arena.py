"""Caller-owned device buffers between two zones of known bytes: what libedsx_guard.so does for the library's own
buffers, done for the memory a caller hands to the device-resident entry points.

One torch.uint8 tensor holds [64 KiB front zone | payload of exactly N bytes | 64 KiB back zone].  Zones and payload
are pre-filled with chosen bytes, the payload pointer can sit `offset` bytes behind a 256-byte boundary, and check()
downloads both zones and reports the first and the last byte that changed, relative to the payload's edge, in the
wording of edsx_guard_check: +0 is the first byte behind the payload, -1 the last byte in front of it.  64 KiB is the
guard build's reach; the widest single store of the library is 4 KB per workgroup.

What it sees: stores outside the payload, payload bytes a call left unwritten (run it under two fills and compare),
and results that depend on the bytes around an input (run it under several zone fills).  What it cannot see: a LOAD
outside the payload whose value is masked out or never reaches an output is as invisible here as in the guard build,
and so is a store further than 64 KiB away or one that happens to write the fill byte (hence several fills).

Every torch operation here runs on torch's current stream: a test that drives the library on a stream of its own
wraps its arena work in `with torch.cuda.stream(s)`.  No GPU code of its own; imported by GPU tests only."""
import numpy as np

ZONE = 64 << 10
ALIGN = 256


class Arena:
    def __init__(self, nbytes, fill=0x00, offset=0, front=None, back=None, name="arena", device="cuda:0"):
        import torch
        assert 0 <= offset < ALIGN and nbytes >= 0
        self.n, self.name, self.offset = int(nbytes), name, offset
        self.fill = fill & 0xff
        self.front_fill = self.fill if front is None else front & 0xff
        self.back_fill = self.fill if back is None else back & 0xff
        self.buf = torch.empty(ZONE + 2 * ALIGN + self.n + ZONE, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        self.start = (base + ZONE + ALIGN - 1) // ALIGN * ALIGN + offset - base        # payload's index in buf
        assert self.start >= ZONE and self.start + self.n + ZONE <= self.buf.numel()
        self.buf[self.start - ZONE:self.start].fill_(self.front_fill)
        self.payload.fill_(self.fill)
        self.buf[self.start + self.n:self.start + self.n + ZONE].fill_(self.back_fill)

    @property
    def ptr(self):
        """Device address of the payload's first byte ((ptr - offset) % 256 == 0)."""
        return self.buf.data_ptr() + self.start

    @property
    def payload(self):
        return self.buf[self.start:self.start + self.n]

    def upload(self, data):
        import torch
        assert len(data) == self.n
        if self.n:
            self.payload.copy_(torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()))
        return self

    def download(self):
        return self.payload.cpu().numpy().tobytes()

    def check(self):
        """-> one line per dirty zone (none: []), the front zone first:
        "<name> <bytes> bytes, <front|back> zone, offsets <first>..<last>, fill <xx>, found <xx xx ..>"."""
        z = self.buf[self.start - ZONE:self.start + self.n + ZONE].cpu().numpy()
        out = []
        for which, zone, fill, edge in (("front", z[:ZONE], self.front_fill, -ZONE), ("back", z[ZONE + self.n:], self.back_fill, 0)):
            bad = np.flatnonzero(zone != fill)
            if bad.size:
                found = " ".join("%02x" % b for b in zone[bad[:8]])
                out.append("%s %d bytes, %s zone, offsets %+d..%+d, fill %02x, found %s"
                           % (self.name, self.n, which, edge + int(bad[0]), edge + int(bad[-1]), fill, found))
        return out

    def assert_clean(self):
        lines = self.check()
        assert not lines, "\n".join(lines)
