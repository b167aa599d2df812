#!/usr/bin/env python3
"""Makes tests/golden/ed25519_openssl.json with the LOCAL openssl binary (3.x): for each entry a seed, the public key openssl derives
from it, a message and the signature `openssl pkeyutl -sign -rawin` makes (Ed25519 is deterministic: an independent known answer for
signer and verifier alike).  The tests read only the JSON; run this by hand to regenerate it:  python tests/golden/make_ed25519_openssl.py"""
import hashlib
import json
import subprocess
import tempfile
from pathlib import Path

LENGTHS = [0, 1, 3, 47, 48, 49, 111, 112, 113, 127, 128, 129, 736, 2144]
EXTRA = [32, 64, 255, 1023]
PKCS8_PREFIX = bytes.fromhex("302e020100300506032b657004220420")      # PrivateKeyInfo { v0, id-Ed25519, OCTET STRING { OCTET STRING seed } }
RFC8032_TEST1 = {
    "seed": "9d61b19deffd5a60ba844af492ec2cc44449c5697b326919703bac031cae7f60",
    "public_key": "d75a980182b10ab7d54bfed3c964073a0ee172f3daa62325af021a68f707511a",
    "message": "",
    "signature": "e5564300c360ac729086e2cc806e828a84877f1eb8e5d974d873e065224901555fb8821590a33bacc61e39701cf9b46bd25bf5f0595bbe24655141438e7a100b",
}


def stream(tag: str, n: int) -> bytes:
    out, i = b"", 0
    while len(out) < n:
        out += hashlib.sha512(f"ed25519-openssl-fixture/{tag}/{i}".encode()).digest()
        i += 1
    return out[:n]


def openssl(*args):
    return subprocess.run(["openssl", *args], check=True, capture_output=True).stdout


def main():
    version = openssl("version").decode().strip()
    entries = []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        for k, n in enumerate(LENGTHS + LENGTHS + EXTRA):
            if n == 0:
                # the openssl 3.0 command line cannot sign an empty file ("Could not allocate 0 bytes for oneshot sign/verify buffer"):
                # length 0 is RFC 8032 section 7.1 TEST 1, once
                if k == 0:
                    entries.append(dict(RFC8032_TEST1, source="RFC 8032 7.1 TEST 1"))
                continue
            seed, msg = stream(f"seed/{k}", 32), stream(f"msg/{k}", n)
            (tmp / "key.der").write_bytes(PKCS8_PREFIX + seed)
            (tmp / "msg").write_bytes(msg)
            pub = openssl("pkey", "-inform", "DER", "-in", str(tmp / "key.der"), "-pubout", "-outform", "DER")[-32:]
            openssl("pkeyutl", "-sign", "-rawin", "-keyform", "DER", "-inkey", str(tmp / "key.der"), "-in", str(tmp / "msg"), "-out", str(tmp / "sig"))
            sig = (tmp / "sig").read_bytes()
            assert len(pub) == 32 and len(sig) == 64
            # openssl's own verdict on what it made
            (tmp / "pub.der").write_bytes(bytes.fromhex("302a300506032b6570032100") + pub)
            openssl("pkeyutl", "-verify", "-rawin", "-pubin", "-keyform", "DER", "-inkey", str(tmp / "pub.der"), "-in", str(tmp / "msg"),
                    "-sigfile", str(tmp / "sig"))
            entries.append({"seed": seed.hex(), "public_key": pub.hex(), "message": msg.hex(), "signature": sig.hex(), "source": "openssl"})
    out = Path(__file__).with_name("ed25519_openssl.json")
    out.write_text(json.dumps({"made_by": version, "entries": entries}, indent=1) + "\n")
    print(f"{out}: {len(entries)} entries by {version}")


if __name__ == "__main__":
    main()
