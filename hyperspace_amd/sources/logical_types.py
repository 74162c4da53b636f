"""One engine representation per parquet logical type.

Every read path (native host read, device read, pyarrow fallback)
consults this module, so the dtype and values of a column never depend on
the path its file happened to take (codec, encoding, footer statistics).
The same table is written out in docs/DESIGN.md ("Logical types").

    parquet column                              engine tensor
    ------------------------------------------  -------------------------
    INT32 / INT64 / FLOAT / DOUBLE, plain       int32/int64/float32/float64
    INT(8, signed), INT(16, signed)             int8, int16
    INT(8, unsigned), INT(16, unsigned)         int32
    INT(32, unsigned)                           int64, zero-extended
    INT(64, unsigned)                           refused
    DATE                                        int32 days
    DECIMAL p <= 18 (INT32 / INT64 / FLBA)      int64 unscaled
    TIMESTAMP ms / us / ns                      int64 in the file's unit
    UTF-8 BYTE_ARRAY, BOOLEAN                   unchanged
    TIME, BYTE_ARRAY without a string
    annotation, DECIMAL p > 18                  refused

"Refused" raises HyperspaceException naming the column and the type,
before anything is read, allocated or launched.

The native decoders keep working on the PHYSICAL type (the page payload
is the little-endian physical buffer); a column whose engine dtype
differs carries a ``Conv`` and is converted once, after assembly.
"""

from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import numpy as np

from ..exceptions import HyperspaceException


class Conv(NamedTuple):
    """Physical buffer -> engine tensor, for the few annotations where
    the two differ: narrow INT32 to int8/int16, sign-extend an INT32
    decimal, zero-extend an INT32 holding uint32."""
    dtype: np.dtype
    zero_extend: bool = False


_INT32_CONVS = {
    "INT_8": Conv(np.dtype("int8")),
    "INT_16": Conv(np.dtype("int16")),
    "UINT_32": Conv(np.dtype("int64"), True),
}
_STRING_ANNOTATIONS = ("STRING", "UTF8")
_TIME_ANNOTATIONS = ("TIME", "TIME_MILLIS", "TIME_MICROS")


def refuse(name: str, what: str, why: str):
    raise HyperspaceException(
        f"Unsupported type for column '{name}': {what} ({why})")


def parquet_conv(col_schema, name: Optional[str] = None) -> Optional[Conv]:
    """The conversion a parquet leaf needs after its physical decode
    (None: the physical buffer IS the engine tensor); raises
    HyperspaceException for a refused type.  ``col_schema`` is a pyarrow
    parquet ColumnSchema."""
    name = name or col_schema.path
    phys = col_schema.physical_type
    logical = col_schema.logical_type.type
    converted = col_schema.converted_type
    if logical in _TIME_ANNOTATIONS or converted in _TIME_ANNOTATIONS:
        refuse(name, "TIME", "time-of-day has no engine representation")
    if logical == "DECIMAL" or converted == "DECIMAL":
        if col_schema.precision > 18:
            refuse(name, f"DECIMAL({col_schema.precision},"
                   f"{col_schema.scale})",
                   "decimal precision > 18 does not fit the unscaled "
                   "int64 representation")
        return Conv(np.dtype("int64")) if phys == "INT32" else None
    if phys == "INT32":
        return _INT32_CONVS.get(converted)
    if phys == "INT64" and converted == "UINT_64":
        refuse(name, "INT(64, unsigned)",
               "Spark maps it to decimal(20,0), past the p <= 18 limit")
    if phys == "BYTE_ARRAY" and logical not in _STRING_ANNOTATIONS \
            and converted not in _STRING_ANNOTATIONS:
        refuse(name, "BYTE_ARRAY without a string annotation",
               "raw binary has no engine representation")
    return None


def parquet_convs(pf_schema, want=None) -> Dict[int, Conv]:
    """{leaf index: Conv} over the wanted leaves of a parquet schema
    (``want``: lower-cased leaf paths, None = all).  Raises for the first
    refused leaf — the one check every read path runs before it reads."""
    out: Dict[int, Conv] = {}
    for i in range(len(pf_schema)):
        col = pf_schema.column(i)
        if want is not None and col.path.lower() not in want:
            continue
        conv = parquet_conv(col, col.path)
        if conv is not None:
            out[i] = conv
    return out


def check_parquet_file(path: str, columns=None) -> None:
    """Raise if ``path`` holds a refused type among ``columns`` (a dotted
    request may name a struct: its leaves are checked)."""
    import pyarrow.parquet as pq
    sch = pq.ParquetFile(path).schema
    want = None
    if columns is not None:
        want = [c.lower() for c in columns]
    for i in range(len(sch)):
        col = sch.column(i)
        p = col.path.lower()
        if want is None or any(p == w or p.startswith(w + ".")
                               for w in want):
            parquet_conv(col, col.path)


def convert_np(arr: np.ndarray, conv: Optional[Conv]) -> np.ndarray:
    """Physical numpy buffer -> engine array."""
    if conv is None:
        return arr
    if conv.zero_extend:
        return np.ascontiguousarray(arr).view(np.uint32).astype(conv.dtype)
    return arr.astype(conv.dtype)


def to_storage_np(arr: np.ndarray, phys: np.dtype) -> np.ndarray:
    """Engine array -> the physical dtype the device read stores before
    its convert step: the exact inverse of convert_np on every value a
    file of that type can hold (int64 -> int32 keeps the low 32 bits)."""
    return arr.astype(phys, copy=False)


def convert_torch(t, conv: Conv):
    """Device twin of convert_np: one elementwise torch op on the
    current stream."""
    import torch
    if conv.zero_extend:
        return t.to(torch.int64).bitwise_and_(0xFFFFFFFF)
    return t.to({np.dtype("int8"): torch.int8,
                 np.dtype("int16"): torch.int16,
                 np.dtype("int64"): torch.int64}[conv.dtype])


def arrow_engine_type(name: str, typ):
    """The arrow type a column casts to before it becomes a tensor (None:
    as it is); raises for a refused arrow type.  The arrow-side reading
    of the same table, for the pyarrow fallback and non-parquet
    sources."""
    import pyarrow as pa
    t = pa.types
    if t.is_uint8(typ) or t.is_uint16(typ):
        return pa.int32()
    if t.is_uint32(typ):
        return pa.int64()
    if t.is_uint64(typ):
        refuse(name, "uint64",
               "Spark maps it to decimal(20,0), past the p <= 18 limit")
    if t.is_date(typ):
        return pa.int32()
    if t.is_time(typ):
        refuse(name, str(typ), "time-of-day has no engine representation")
    if t.is_binary(typ) or t.is_large_binary(typ) or \
            t.is_fixed_size_binary(typ):
        refuse(name, str(typ), "raw binary has no engine representation")
    return None
