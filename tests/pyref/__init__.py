"""pyref -- a second judge of the protocol layer, in plain Python integers (test infrastructure only).

Every other expected value of the suite comes from the C oracle (oracle/*.c).  This package restates the VERIFIERS of
slowli/elastic-elgamal a second time, from the Rust source (file and line are cited where a rule is taken), so that a reading of
the reference that the oracle's prover and verifier share is still judged by something that does not share it.

Independent of: the oracle, the product, numpy, torch, ctypes -- standard library only, nothing imported from outside the
package (tests/test_pyref_cpu.py walks the package with `ast` and asserts it).  Field and group arithmetic follow RFC 9496 and the
Edwards addition law, the protocol follows src/proofs/*.rs, src/app/*.rs, src/keys/impls.rs and src/sharing/key_set.rs, the packed
layouts and status words follow include/eg_hip.h.

NOT independent: the transcript framing (merlin.py), see its docstring.

Modules: field (mod p, mod l, SQRT_RATIO_M1), ristretto (points, decode / encode, products), keccak, merlin, protocol (the
reference's verifiers on decoded objects), packed (the project's packed forms -> status words, tallies), objects (the reference's
serde object form).
"""
