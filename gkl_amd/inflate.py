"""Host-side mirror of the reference's plugin class ``com.intel.gkl.compression.IntelInflater`` (reference
src/main/java/com/intel/gkl/compression/IntelInflater.java): same method names, argument checks (:126-175) and exception
messages, and the RuntimeException messages the JNI layer raises for a bad stream (IntelInflater.cc:179-210).  It talks
to the C ABI of include/inflate/gkl_hip_inflate.h and never decodes anything itself.

One stream per ``inflate`` call: the call inflates the input set by ``setInput`` from its first bit into ``b[off:off+len]``
and carries no state to the next call, which is how htsjdk's BlockGunzipper uses the class (reset, setInput, one inflate
into a buffer that holds the whole BGZF block).  One stream per launch is the slow way to use a GPU (README, "Inflate");
the batch entry points of ``native.InflateContext`` are the ones that pay."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import native
from .errors import ArrayIndexOutOfBoundsException, IllegalArgumentException, NullPointerException, RuntimeException

# what IntelInflater.cc raises for the ISA-L code that matches each stream status
_MESSAGES = {
    native.INFLATE_INVALID_BLOCK: "Invalid deflate block found.",
    native.INFLATE_INVALID_SYMBOL: "Invalid deflate symbol found.",
    native.INFLATE_INVALID_LOOKBACK: "Invalid lookback distance found.",
}


class IntelInflater:
    NATIVE_LIBRARY_NAME = "gkl_compression"

    def __init__(self, nowrap: bool = True):
        if not nowrap:
            raise IllegalArgumentException("ZLIB format is not supported at this time with Intel GKL")
        self.nowrap = nowrap
        self._ctx: Optional[native.InflateContext] = None
        self._input = None
        self._input_off = 0
        self._input_len = 0
        self._finished = False

    def load(self, tempDir=None) -> bool:
        """True when the library and a gfx950 device are usable."""
        try:
            if self._ctx is None:
                self._ctx = native.InflateContext()
            return True
        except RuntimeException:
            return False

    def reset(self) -> None:
        if self._ctx is None and not self.load():
            raise RuntimeException("no gfx950 device: the inflater has no CPU path")
        self._input = None
        self._input_len = 0
        self._finished = False

    def setInput(self, b, off: int = 0, len_: Optional[int] = None) -> None:
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

    def inflate(self, b, off: int = 0, len_: Optional[int] = None) -> int:
        """Inflates the input into b[off:off+len] (b: a bytearray or a writable uint8 buffer); returns the bytes written."""
        if b is None:
            raise NullPointerException("Output buffer is null")
        if len_ is None:
            len_ = len(b) - off
        if off < 0:
            raise ArrayIndexOutOfBoundsException("Offset value is less than zero")
        if len_ < 0:
            raise ArrayIndexOutOfBoundsException("Length value is less than zero")
        if off > len(b) - len_:
            raise ArrayIndexOutOfBoundsException("Length value exceeds permissible range")
        if self._input is None or self._input_len == 0:
            raise NullPointerException("Input buffer is null")
        if self._ctx is None:
            self.reset()
        stream = bytes(self._input[self._input_off:self._input_off + self._input_len])
        outs, _, statuses, consumed = self._ctx.inflate_batch([stream], [len_])
        status = statuses[0]
        if status in _MESSAGES:
            raise RuntimeException(_MESSAGES[status])
        n = len(outs[0])
        np.frombuffer(b, dtype=np.uint8)[off:off + n] = np.frombuffer(outs[0], dtype=np.uint8)
        # the reference: finished = the decoder returned without an error and took all of the input
        self._finished = status == native.INFLATE_END_INPUT or (status == native.INFLATE_OK and consumed[0] == self._input_len)
        return n

    def finished(self) -> bool:
        return self._finished

    def end(self) -> None:
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    close = end
