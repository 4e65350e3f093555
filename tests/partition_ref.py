"""A plain-Python restatement of src/partition.rs and of sigma_polynomials (plonk_util.rs:264-280) on big integers: the checker of the
sigma tests.  Written from the reference text, with a Vec as a list and a HashMap as a dict, line for line; it shares nothing with
the mirror in plonky_amd.api.  A target is ("wire", gate, input) or ("virtual", index); a wire is (gate, input).
"""
NUM_WIRES = 9          # plonk.rs:21
NUM_ROUTED_WIRES = 6   # plonk.rs:22


class TargetPartitionsRef:
    def __init__(self):                                   # partition.rs:18-23
        self.partitions = []
        self.indices = {}

    def add_partition(self, target):                      # partition.rs:30-34
        index = len(self.partitions)
        self.partitions.append([target])
        self.indices[target] = index

    def merge(self, a, b):                                # partition.rs:38-52
        a_index = self.indices[a]
        b_index = self.indices[b]
        if a_index != b_index:
            a_partition = self.partitions[a_index][:]     # .clone(): the original list stays at a_index
            b_partition = self.partitions[b_index]
            for a_sibling in a_partition:
                self.indices[a_sibling] = b_index
            b_partition += a_partition                    # append

    def to_wire_partitions(self):                         # partition.rs:54-81
        partitions = []
        indices = {}
        for old_partition in self.partitions:
            new_partition = []
            for target in old_partition:
                if target[0] == "wire":
                    new_partition.append((target[1], target[2]))
            partitions.append(new_partition)
        for target, index in self.indices.items():
            if target[0] == "wire":
                indices[(target[1], target[2])] = index
        result = WirePartitionsRef(partitions, indices)
        result.assert_valid()
        return result


class WirePartitionsRef:
    def __init__(self, partitions, indices):
        self.partitions = partitions
        self.indices = indices

    def assert_valid(self):                               # partition.rs:90-102
        for partition in self.partitions:
            for (_gate, inp) in partition:
                if inp >= NUM_ROUTED_WIRES:
                    assert len(partition) == 1, "Non-routed wires should not be in a partition containing other wires"

    def get_neighbor(self, wire):                         # partition.rs:108-118
        partition = self.partitions[self.indices[wire]]   # KeyError: the reference's index panic
        n = len(partition)
        for i in range(n):
            if partition[i] == wire:
                neighbor_index = (i + 1) % n
                return partition[neighbor_index]
        raise AssertionError("Wire not found in the expected partition")

    def to_sigma(self):                                   # partition.rs:122-136
        assert len(self.indices) % NUM_WIRES == 0
        num_all_wires = len(self.indices)
        num_gates = num_all_wires // NUM_WIRES
        sigma = []
        for inp in range(NUM_ROUTED_WIRES):
            for gate in range(num_gates):
                n_gate, n_inp = self.get_neighbor((gate, inp))
                sigma.append(n_inp * num_gates + n_gate)
        return sigma


def sigma_polynomials_ref(sigma, degree, subgroup_generator, k_is, p):
    """plonk_util.rs:264-280 on integers modulo p: chunks of `degree`, element x -> k_is[x / degree] * g^(x % degree)"""
    chunks = [sigma[i:i + degree] for i in range(0, len(sigma), degree)]
    return [[k_is[x // degree] * pow(subgroup_generator, x % degree, p) % p for x in chunk] for chunk in chunks]


def csr_to_wire_partitions(members, offsets, degree):
    """the flattened form back to a WirePartitionsRef (one partition per offsets interval, a wire's index the LAST interval that lists
    it, as repeated inserts into a HashMap would leave it)"""
    partitions = []
    indices = {}
    for q in range(len(offsets) - 1):
        part = [(int(m) % degree, int(m) // degree) for m in members[offsets[q]:offsets[q + 1]]]
        for w in part:
            indices[w] = q
        partitions.append(part)
    return WirePartitionsRef(partitions, indices)


def status_words_ref(members, offsets, degree):
    """the three status words of plk_plonk_sigma_dev from their definitions (include/plonky_hip.h), by counting"""
    counts = {}
    lonely = out_of_range = 0
    for q in range(len(offsets) - 1):
        part = [int(m) for m in members[offsets[q]:offsets[q + 1]]]
        for m in part:
            if m >= NUM_WIRES * degree:
                out_of_range += 1
            elif m >= NUM_ROUTED_WIRES * degree:
                lonely += len(part) > 1
            else:
                counts[m] = counts.get(m, 0) + 1
    missing = sum(1 for w in range(NUM_ROUTED_WIRES * degree) if w not in counts)
    surplus = sum(c - 1 for c in counts.values())
    return [missing + surplus, lonely, out_of_range]
