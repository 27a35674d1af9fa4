"""Host-side mirror of the reference's plugin class ``com.intel.gkl.compression.IntelDeflater`` (reference
src/main/java/com/intel/gkl/compression/IntelDeflater.java): same method names, constructor checks (:89-97), argument
checks (:150-163, :191-203) and exception messages, and the RuntimeException the JNI layer raises when the stream does
not fit the output buffer (IntelDeflater.cc, STATELESS_OVERFLOW: "Output buffer too small.").  It talks to the C ABI of
include/deflate/gkl_hip_deflate.h and never encodes anything itself.

One stream per ``deflate`` call: after ``finish()`` the call deflates the input set by ``setInput`` into ``b[0:len]`` as
one whole raw-deflate stream, which is how htsjdk's BlockCompressedOutputStream uses the class (reset, setInput, finish,
one deflate into a buffer that holds the whole BGZF block).  One stream per launch is the slow way to use a GPU
(README, "Deflate"); the batch entry points of ``native.DeflateContext`` are the ones that pay.

Built levels: 0 (stored blocks), 1 (one-entry hash table, greedy) and 3 to 8 (hash chains of depth 4 to 128, minimum
match 3, lazy selection from level 4 on).  The reference sends levels 1 and 2 to ISA-L and the others to zlib; here
levels 2, 9 and -1 (the default) are refused at ``reset()``.  The stream is valid raw deflate, not the reference's byte
sequence."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import native
from .errors import ArrayIndexOutOfBoundsException, IllegalArgumentException, NullPointerException, RuntimeException

DEFAULT_COMPRESSION = -1
DEFAULT_STRATEGY = 0
BUILT_LEVELS = (0, 1, 3, 4, 5, 6, 7, 8)


class IntelDeflater:
    NATIVE_LIBRARY_NAME = "gkl_compression"

    def __init__(self, level: int = DEFAULT_COMPRESSION, nowrap: bool = True):
        if (level < 0 or level > 9) and level != DEFAULT_COMPRESSION:
            raise IllegalArgumentException("Illegal compression level")
        if level in (1, 2) and not nowrap:
            raise IllegalArgumentException("Compression configuration requested not supported")
        self.level = level
        self.nowrap = nowrap
        self.strategy = DEFAULT_STRATEGY
        self._ctx: Optional[native.DeflateContext] = None
        self._input = None
        self._input_off = 0
        self._input_len = 0
        self._end_of_stream = False
        self._finished = False

    def load(self, tempDir=None) -> bool:
        """True when the library and a gfx950 device are usable."""
        try:
            if self._ctx is None:
                self._ctx = native.DeflateContext()
            return True
        except RuntimeException:
            return False

    def reset(self) -> None:
        if self.level not in BUILT_LEVELS or not self.nowrap:
            raise RuntimeException(f"compression level {self.level} (nowrap={self.nowrap}) is not built: raw deflate at levels 0, 1 and 3 to 8 is")
        if self._ctx is None and not self.load():
            raise RuntimeException("no gfx950 device: the deflater has no CPU path")
        self._input = None
        self._input_len = 0
        self._end_of_stream = False
        self._finished = False

    def setInput(self, b, off: int = 0, len_: Optional[int] = None) -> None:
        """The reference's setInput keeps ``b`` and ``len`` and forgets ``off`` (the native side always reads from the
        buffer's first byte); the mirror honours ``off``."""
        if self._ctx is None:
            self.reset()
        if b is None:
            raise NullPointerException("Input buffer is null")
        if len_ is None:
            len_ = len(b) - off
        if off < 0:
            raise ArrayIndexOutOfBoundsException("Offset value is less than zero")
        if len_ < 0:
            raise ArrayIndexOutOfBoundsException("Length value is less than zero")
        if off > len(b) - len_:
            raise ArrayIndexOutOfBoundsException("Length value exceeds permissible range")
        self._input, self._input_off, self._input_len = b, off, len_

    def finish(self) -> None:
        self._end_of_stream = True

    def deflate(self, b, off: int = 0, len_: Optional[int] = None) -> int:
        """Deflates the whole input into b[0:len] (b: a bytearray or a writable uint8 buffer); returns the bytes written."""
        if b is None:
            raise NullPointerException("Output buffer is null")
        if off != 0:
            raise IllegalArgumentException("The only accepted offset value is 0")
        if len_ is None:
            len_ = len(b)
        if len_ <= 0:
            raise ArrayIndexOutOfBoundsException("Length value is less or equal than zero")
        if self._input is None or self._input_len == 0:
            raise NullPointerException("Input buffer is null")
        if not self._end_of_stream:
            raise RuntimeException("deflate before finish(): the mirror writes one whole stream per call")
        if self._ctx is None:
            self.reset()
        data = bytes(self._input[self._input_off:self._input_off + self._input_len])
        outs, _, statuses = self._ctx.deflate_batch([data], self.level, [min(len_, len(b))])
        if statuses[0] == native.DEFLATE_OUT_OVERFLOW:
            raise RuntimeException("Output buffer too small.")
        n = len(outs[0])
        np.frombuffer(b, dtype=np.uint8)[:n] = np.frombuffer(outs[0], dtype=np.uint8)
        self._finished = True
        return n

    def finished(self) -> bool:
        return self._finished

    def end(self) -> None:
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    close = end
