"""The column-global string order hy_string_dictionary_order computes, restated on the host: every chunk's dictionary entry -> its dense
rank among the distinct strings of ALL chunks, in std::string order (bytes unsigned, a prefix first), which is Python's order of bytes."""


def column_order(dictionaries):
    """dictionaries: per chunk a list of byte strings (sorted, duplicate-free) -> (per chunk the list of ranks, n_distinct)."""
    distinct = sorted({entry for dictionary in dictionaries for entry in dictionary})
    rank = {entry: i for i, entry in enumerate(distinct)}
    return [[rank[entry] for entry in dictionary] for dictionary in dictionaries], len(distinct)
