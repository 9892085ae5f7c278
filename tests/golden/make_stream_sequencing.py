"""Records tests/golden/stream_sequencing.npz: the answers of the sizing / scheduling queries of the C ABI over the grid of
tests/test_stream_sequencing.py, from a library built at the commit whose behaviour is to be kept:

    python tests/golden/make_stream_sequencing.py /path/to/that/checkout/tpnet_amd/libtpnet_hip.so

No device is needed.  The table is plain integers: the grid's rows and one uint64 answer per row."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import test_stream_sequencing as T  # noqa: E402


def main():
    lib = C.CDLL(os.path.abspath(sys.argv[1]))
    i32, i64, u32, sz = C.c_int32, C.c_int64, C.c_uint32, C.c_size_t
    for name, res, args in (("tpnet_stream_workspace_bytes", sz, [i64, i32, i32, i64, i64]),
                            ("tpnet_stream_workspace_bytes_capped", sz, [i64, i32, i32, i64, i64, sz]),
                            ("tpnet_stream_schedule", C.c_int, [i64, i32, i32, i64, i64, u32, sz]),
                            ("tpnet_wshard_workspace_bytes", sz, [i64, i32, i32, i64, i64, i32, i32])):
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    rows, out = T.answers(lib)
    path = os.path.join(HERE, "stream_sequencing.npz")
    np.savez_compressed(path, columns=np.asarray(T.COLUMNS), rows=rows, answers=out)
    print(path, rows.shape, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
