"""Rescue on Python integers, restated from the reference line by line: Field::kth_root (field.rs:346-375), the Cauchy MDS matrix
(mds.rs:43-77), rescue_permutation and rescue_sponge (rescue.rs:40-88), recommended_rounds (rescue.rs:123-125) and the Challenger
(plonk_challenger.rs:20-109).  Values are canonical integers; the callers convert to and from Montgomery limbs.

The round constants are NOT the reference's (ChaCha8Rng::seed_from_u64(1337), rescue.rs:105): they are seeded values from
oracle.bigint_ref.rand_field_limbs, which is also what the tests hand to the library."""
from oracle import bigint_ref as br

RESCUE_SPONGE_WIDTH = 4  # plonk.rs
RESCUE_SPONGE_RATE = 3
ALPHA = {0: 5, 1: 5, 2: 11, 3: 5, 4: 5, 5: 5}  # F::ALPHA; bls12_377_scalar.rs:169 holds the Montgomery limbs of 11


def kth_root_exponent(p, k):
    """field.rs:354-369: the first n in 1 ..= k with k | p + n (p - 1); None where the reference panics."""
    p_minus_1 = p - 1
    n = 0
    numerator = p_minus_1 + 1
    while n < k:
        n += 1
        numerator += p_minus_1
        if numerator % k == 0:
            return (numerator // k) % p_minus_1
    return None


def kth_root(p, x, k):
    return pow(x, kth_root_exponent(p, k), p)


def mds_matrix(p, n):
    """mds.rs:63-76: the Cauchy matrix with x_r = n + r, y_c = c."""
    return [[pow((n + r - c) % p, -1, p) for c in range(n)] for r in range(n)]


def apply_mds(p, inputs):  # mds.rs:43-53
    n = len(inputs)
    mds = mds_matrix(p, n)
    return [sum(mds[r][c] * inputs[c] for c in range(n)) % p for r in range(n)]


def recommended_rounds(width, security_bits):  # rescue.rs:123-125
    return max(-(-security_bits // (2 * width)), 10)


def constants(field, width, rounds, seed=1337):
    """rounds x (step A, step B) x width canonical values: the seeded stand-in for generate_rescue_constants"""
    f = br.FIELDS[field]
    flat = [f.from_mont(br.limbs_to_int(l)) for l in br.rand_field_limbs(f, seed, rounds * 2 * width)]
    return [(flat[(2 * r) * width:(2 * r + 1) * width], flat[(2 * r + 1) * width:(2 * r + 2) * width]) for r in range(rounds)]


def constants_limbs(field, consts):
    """the same constants as the library takes them: rounds x 2 x width rows of Montgomery limbs"""
    f = br.FIELDS[field]
    return [f.mont_limbs(v) for a, b in consts for v in a + b]


def rescue_permutation(field, state, consts):  # rescue.rs:70-88
    p, alpha = br.FIELDS[field].p, ALPHA[field]
    d = kth_root_exponent(p, alpha)
    state = list(state)
    for step_a, step_b in consts:
        state = [pow(x, d, p) for x in state]
        state = apply_mds(p, state)
        state = [(a + b) % p for a, b in zip(state, step_a)]
        state = [pow(x, alpha, p) for x in state]
        state = apply_mds(p, state)
        state = [(a + b) % p for a, b in zip(state, step_b)]
    return state


def rescue_sponge(field, inputs, num_outputs, consts):  # rescue.rs:40-68
    p = br.FIELDS[field].p
    rate, capacity = 3, 1
    state = [0] * (rate + capacity)
    for at in range(0, len(inputs), rate):
        chunk = inputs[at:at + rate]
        for i in range(len(chunk)):
            state[i] = (state[i] + chunk[i]) % p
        state = rescue_permutation(field, state, consts)
    outputs = []
    while True:
        for i in range(rate):
            outputs.append(state[i])
            if len(outputs) == num_outputs:
                return outputs
        state = rescue_permutation(field, state, consts)


class Challenger:
    """plonk_challenger.rs:20-109, as it is written: get_challenge pops from the END of the output buffer, and absorb_buffered_inputs
    refills that buffer from the state on every call - so challenges drawn with nothing observed in between are equal."""

    def __init__(self, field, consts):
        self.field, self.consts = field, consts
        self.sponge_state = [0] * RESCUE_SPONGE_WIDTH
        self.input_buffer = []
        self.output_buffer = []

    def clone(self):
        c = Challenger(self.field, self.consts)
        c.sponge_state, c.input_buffer, c.output_buffer = list(self.sponge_state), list(self.input_buffer), list(self.output_buffer)
        return c

    def observe_element(self, element):
        self.output_buffer = []
        self.input_buffer.append(element)

    def observe_elements(self, elements):
        for e in elements:
            self.observe_element(e)

    def observe_affine_point(self, point):
        self.observe_element(point[0])
        self.observe_element(point[1])

    def observe_affine_points(self, points):
        for pt in points:
            self.observe_affine_point(pt)

    def get_challenge(self):
        self._absorb_buffered_inputs()
        if not self.output_buffer:  # never taken: the line above has just filled the buffer (plonk_challenger.rs:66-70)
            self.sponge_state = rescue_permutation(self.field, self.sponge_state, self.consts)
            self.output_buffer = self.sponge_state[:RESCUE_SPONGE_RATE]
        return self.output_buffer.pop()

    def get_2_challenges(self):
        return self.get_challenge(), self.get_challenge()

    def get_3_challenges(self):
        return self.get_challenge(), self.get_challenge(), self.get_challenge()

    def get_n_challenges(self, n):
        return [self.get_challenge() for _ in range(n)]

    def _absorb_buffered_inputs(self):
        p = br.FIELDS[self.field].p
        for at in range(0, len(self.input_buffer), RESCUE_SPONGE_RATE):
            chunk = self.input_buffer[at:at + RESCUE_SPONGE_RATE]
            for i, v in enumerate(chunk):
                self.sponge_state[i] = (self.sponge_state[i] + v) % p
            self.sponge_state = rescue_permutation(self.field, self.sponge_state, self.consts)
        self.output_buffer = self.sponge_state[:RESCUE_SPONGE_RATE]
        self.input_buffer = []
