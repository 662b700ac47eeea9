"""Reader for the PNG / APNG files hostio writes (8-bit RGB, filter type 0 on every row): chunk walk with CRC check, inflate,
strip the filter bytes.  Test helper; no PIL."""
import struct
import zlib

import numpy as np


def chunks(data):
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, out = 8, []
    while pos < len(data):
        n, = struct.unpack('>I', data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff, tag
        out.append((tag, body))
        pos += 12 + n
    assert pos == len(data)
    return out


def _rows(stream, h, w):
    raw = np.frombuffer(zlib.decompress(stream), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3)


def read_frames(path):
    """Every frame of a PNG (one) or APNG file as uint8 (H, W, 3) arrays."""
    cs = chunks(open(path, 'rb').read())
    w, h, depth, colour, _, _, interlace = struct.unpack('>IIBBBBB', cs[0][1])
    assert cs[0][0] == b'IHDR' and (depth, colour, interlace) == (8, 2, 0)
    frames = [_rows(b''.join(b for t, b in cs if t == b'IDAT'), h, w)]
    frames += [_rows(b[4:], h, w) for t, b in cs if t == b'fdAT']
    declared = [struct.unpack('>II', b)[0] for t, b in cs if t == b'acTL']
    assert declared in ([], [len(frames)])
    return frames


def read_png(path):
    frames = read_frames(path)
    assert len(frames) == 1
    return frames[0]
