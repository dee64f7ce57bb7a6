"""The keys hy_string_dictionary_order_pair / hy_string_dictionary_join_ids compute, restated on the host: the dense rank of every dictionary
entry among the distinct strings of BOTH columns' dictionaries, and (rank + 1) << 20 | std::hash & 0xFFFFF."""
from hyrise_amd import join_keys
from string_order_oracle import column_order


def joint_order(left_dicts, right_dicts):
    """left_dicts / right_dicts: per chunk a list of byte strings -> (left's ranks per chunk, right's ranks per chunk, n_distinct)."""
    ranks, n_distinct = column_order(list(left_dicts) + list(right_dicts))
    return ranks[:len(left_dicts)], ranks[len(left_dicts):], n_distinct


def join_ids(left_dicts, right_dicts):
    """-> (left's ids per chunk, right's ids per chunk)"""
    left_ranks, right_ranks, _ = joint_order(left_dicts, right_dicts)
    mask = (1 << join_keys.HASH_BITS) - 1

    def ids(dicts, ranks):
        return [[(rank + 1) << join_keys.HASH_BITS | (join_keys.std_hash_bytes(entry) & mask) for entry, rank in zip(d, r)] for d, r in zip(dicts, ranks)]
    return ids(left_dicts, left_ranks), ids(right_dicts, right_ranks)
