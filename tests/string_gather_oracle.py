"""What hy_string_column_gather and hy_string_ranks_gather produce, restated on the host: the output rows cut into chunks, per chunk the
dictionary sorted(set(...)) over bytes (std::string's order) and the value ids, a NULL row holding the chunk's entry count."""


def encode_chunks(rows, sizes):
    """rows: bytes or None per output row; sizes: rows per output chunk -> (per chunk the dictionary, per chunk the list of value ids)."""
    assert sum(sizes) == len(rows)
    dictionaries, value_ids, begin = [], [], 0
    for size in sizes:
        chunk = rows[begin:begin + size]
        begin += size
        dictionary = sorted({row for row in chunk if row is not None})
        value_id = {entry: i for i, entry in enumerate(dictionary)}
        dictionaries.append(dictionary)
        value_ids.append([len(dictionary) if row is None else value_id[row] for row in chunk])
    return dictionaries, value_ids


def uniform_sizes(n, chunk_rows):
    return [min(chunk_rows, n - begin) for begin in range(0, n, chunk_rows)]


def gathered_rows(chunks, positions):
    """chunks: per source chunk a list of bytes / None; positions: (chunk, offset) pairs, None or (0xFFFFFFFF, 0xFFFFFFFF) for a NULL RowID."""
    rows = []
    for position in positions:
        if position is None or position[1] == 0xFFFFFFFF:
            rows.append(None)
        else:
            rows.append(chunks[position[0]][position[1]])
    return rows


def column_gather(chunks, positions, chunk_rows):
    return encode_chunks(gathered_rows(chunks, positions), uniform_sizes(len(positions), chunk_rows))


def ranks_gather(dictionaries, rank_chunks):
    """dictionaries: the source column's per-chunk dictionaries; rank_chunks: per output chunk a list of ranks / None.  A rank outside
    0 .. n_distinct - 1 gives a NULL row."""
    distinct = sorted({entry for dictionary in dictionaries for entry in dictionary})
    rows = [distinct[r] if r is not None and 0 <= r < len(distinct) else None for chunk in rank_chunks for r in chunk]
    return encode_chunks(rows, [len(chunk) for chunk in rank_chunks])
