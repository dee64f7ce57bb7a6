"""What hy_string_column_substr produces, restated on the host: the reference's SUBSTR (expression_evaluator.cpp:1597-1638) over bytes in
unbounded integers, and the output pair -- the input's own chunks, per chunk the dictionary sorted(set(...)) over the result bytes
(std::string's order) and the value ids, a NULL row holding the chunk's entry count."""
from string_gather_oracle import encode_chunks


def substr(value, start, length):
    """SUBSTR(value, start, length) of bytes: never None."""
    n = len(value)
    if length <= 0:
        return b""
    if start < 0:
        s = start + n
    elif start == 0:
        s, length = 0, length - 1
    else:
        s = start - 1
    e = min(s + length, n)
    s = max(s, 0)
    return value[s:e] if s < n and e > s else b""


def substr_rows(rows, start, length):
    """rows: bytes or None per row; a NULL row stays NULL."""
    return [None if row is None else substr(row, start, length) for row in rows]


def column_substr(chunks, start, length):
    """chunks: per chunk of the input column a list of bytes / None -> (per chunk the dictionary, per chunk the list of value ids)."""
    return encode_chunks([row for chunk in chunks for row in substr_rows(chunk, start, length)], [len(chunk) for chunk in chunks])
