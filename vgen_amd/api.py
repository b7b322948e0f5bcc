"""ctypes binding of include/vgen_hip.h, shaped like the reference's Rust API.

  AddressFormat        src/address.rs:11-24
  GeneratedAddress     src/address.rs:63-72
  Pattern              src/pattern.rs:9-45         (new / matches)
  ScanConfig/Result    src/scanner.rs:17-68
  GpuRunner            src/gpu.rs:116-131,138,535,602   (new / dispatch / await_result)
  scan_gpu_with_runner src/gpu.rs:920-926

The extension is loaded from vgen_amd/libvgen_hip.so (in-tree).  If it is missing the import of
this module fails loudly — nothing here computes an address in Python.
"""
import ctypes
import enum
import os
from dataclasses import dataclass, field
from typing import Callable, List, Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# (_SO_OVERRIDE: a second instance of this module bound to the TEST build of the library — the same sources with the
#  fault-injection hooks compiled in —, pre-set by tests/conftest.py: hooks_api() before it executes the module; never an
#  environment variable, never set in the package itself)
_SO = globals().get("_SO_OVERRIDE") or os.path.join(_HERE, "libvgen_hip.so")


class VgenError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"[vgen status {status}] {message}")
        self.status = status


def library_path():
    return _SO


if not os.path.exists(_SO):
    raise ImportError(f"{_SO} not found: build it with `make -C vgen_amd/csrc` (or __graft_entry__.build()); "
                      "vgen_amd has no pure-Python or CPU fallback")
_L = ctypes.CDLL(_SO)

OK, E_INVALID, E_NODEVICE, E_HIP, E_NOMEM, E_STATE, E_PATTERN, E_RANGE, E_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6, -7, -8


class AddressFormat(enum.IntEnum):
    P2pkh = 0
    P2wpkh = 1
    P2shP2wpkh = 2
    P2tr = 3
    P2pkhUncompressed = 4
    Ethereum = 5
    EthereumContract = 6   # VGEN_FMT_ETHEREUM_CONTRACT: the contract the key's account creates with nonce 0 (not in the reference)
    EthereumCreate2 = 7    # VGEN_FMT_ETHEREUM_CREATE2: a CREATE2 (EIP-1014) address searched by salt (not in the reference)

    def charset_name(self) -> str:
        """AddressFormat::charset_name (src/address.rs:39-45)."""
        return _L.vgen_format_charset_name(int(self)).decode()


# VGEN_FMT_NOSTR: the Nostr public key npub1... (NIP-19), the BIP-340 x-only key itself (not in the reference).  A plain number outside
# the enumeration, as in the header (8 and 9 stay unassigned); every function that takes a format takes it.
FORMAT_NOSTR = 10
# VGEN_FMT_SOLANA: a Solana address, the Ed25519 public key of a 32-byte seed in Base58 (not in the reference).  The key of this format
# is the SEED; 11 stays unassigned.  Scans of such a runner always draw independent seeds (ScanConfig.random_keys is implied).
FORMAT_SOLANA = 12
# VGEN_FMT_ONION: a Tor v3 onion address, the Ed25519 public key of a SCALAR in Base32 (not in the reference).  The key of this format is
# the scalar as 32 little-endian bytes, and scans walk a + 8 i from the base scalar of their seed: the keys of one scan are neighbours.
FORMAT_ONION = 13


def _fmt(v):
    """A format as callers see it: the AddressFormat member, or the plain number of a format outside the enumeration."""
    v = int(v)
    return AddressFormat(v) if v in AddressFormat._value2member_map_ else v


class _Params(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("device", ctypes.c_int32), ("batch_size", ctypes.c_uint32),
                ("format", ctypes.c_uint32), ("frames", ctypes.c_uint32), ("match_cap", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("table_bits", ctypes.c_uint32), ("device_mem_budget_bytes", ctypes.c_uint64)]


class _MemoryInfo(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("table_bits", ctypes.c_uint32), ("frames_bytes", ctypes.c_uint64),
                ("mode_bytes", ctypes.c_uint64), ("table_bytes", ctypes.c_uint64), ("pinned_host_bytes", ctypes.c_uint64),
                ("budget_bytes", ctypes.c_uint64), ("device_free_bytes", ctypes.c_uint64), ("device_total_bytes", ctypes.c_uint64)]


class _Match(ctypes.Structure):
    _fields_ = [("index", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("payload", ctypes.c_uint8 * 32)]


class _ScanConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("format", ctypes.c_uint32), ("count", ctypes.c_uint64),
                ("case_insensitive", ctypes.c_int32), ("has_start", ctypes.c_int32), ("start", ctypes.c_uint8 * 32),
                ("has_end", ctypes.c_int32), ("end", ctypes.c_uint8 * 32), ("seed", ctypes.c_uint64),
                ("shard", ctypes.c_uint32), ("n_shards", ctypes.c_uint32), ("max_batches", ctypes.c_uint64),
                ("checkpoint_path", ctypes.c_char_p), ("checkpoint_interval_ms", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("table_bits_max", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


SCAN_RANDOM_KEYS = 1   # VGEN_SCAN_RANDOM_KEYS
SCAN_BEST = 2          # VGEN_SCAN_BEST


class _Generated(ctypes.Structure):
    _fields_ = [("address", ctypes.c_char * 96), ("wif", ctypes.c_char * 72), ("hex", ctypes.c_char * 72),
                ("format", ctypes.c_uint32), ("key", ctypes.c_uint8 * 32)]


class _ScanResult(ctypes.Structure):
    _fields_ = [("matches", ctypes.POINTER(_Generated)), ("n_matches", ctypes.c_uint64),
                ("operations", ctypes.c_uint64), ("elapsed_secs", ctypes.c_double),
                ("resumed_operations", ctypes.c_uint64), ("complete", ctypes.c_int32), ("failed_shards", ctypes.c_int32)]


_PROGRESS = ctypes.CFUNCTYPE(None, ctypes.c_uint64, ctypes.c_void_p)

_L.vgen_last_error.restype = ctypes.c_char_p
_L.vgen_last_error.argtypes = [ctypes.c_void_p]
_L.vgen_create.argtypes = [ctypes.POINTER(_Params), ctypes.POINTER(ctypes.c_void_p)]
_L.vgen_destroy.argtypes = [ctypes.c_void_p]
_L.vgen_destroy.restype = None
_L.vgen_get_info.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_uint32)] * 3
_L.vgen_filter_compile.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]
_L.vgen_filter_free.argtypes = [ctypes.c_void_p]
_L.vgen_filter_free.restype = None
_L.vgen_filter_matches.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
_L.vgen_filter_device_kind.argtypes = [ctypes.c_void_p]
_L.vgen_filter_dfa_bytes.argtypes = [ctypes.c_void_p]
_L.vgen_pattern_invalid_chars.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t,
                                          ctypes.POINTER(ctypes.c_size_t)]
_L.vgen_pattern_difficulty.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
_L.vgen_format_charset_name.argtypes = [ctypes.c_uint32]
_L.vgen_format_charset_name.restype = ctypes.c_char_p
_L.vgen_provider_resolve.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32), ctypes.c_char_p,
                                     ctypes.c_char_p]
_L.vgen_provider_build_pattern.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t]
_L.vgen_set_filter.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
_L.vgen_clock_probe_start.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
_L.vgen_clock_probe_read.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
_L.vgen_dispatch.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p]
_L.vgen_dispatch_keys.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32]
if hasattr(_L, "vgen_debug_fail_after"):   # only the test build (tests/native/libvgen_hip_hooks.so) has it
    _L.vgen_debug_fail_after.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
_L.vgen_dispatch_random_seed.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64]
_L.vgen_random_key_seed.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p]
_L.vgen_get_resources.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_uint32)] * 3 + [ctypes.c_char_p, ctypes.c_size_t]
_L.vgen_get_memory.argtypes = [ctypes.c_void_p, ctypes.POINTER(_MemoryInfo)]
_L.vgen_dispatch_random.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64]
_L.vgen_random_key.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p]
_L.vgen_wait.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(_Match), ctypes.c_uint32,
                         ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)]
_L.vgen_read_dump.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]
_L.vgen_dump_view.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
_L.vgen_get_topology.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_uint32)] * 3 + [ctypes.POINTER(ctypes.c_int32)]   # streams, hw_queues, priority_levels, oversubscribed
_L.vgen_frame_kernel_ms.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_float)]
_L.vgen_frame_clock.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
_L.vgen_frame_dispatch_ms.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_float)]
_L.vgen_address_from_payload.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
_L.vgen_key_to_wif.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
_L.vgen_key_variant.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
_L.vgen_key_add.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p]
_L.vgen_derive.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
                           ctypes.c_size_t]
_L.vgen_contract_address.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p]
_L.vgen_keccak256.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
_L.vgen_nostr_encode.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
_L.vgen_nostr_decode.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p]
_L.vgen_solana_seed.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p]
_L.vgen_solana_public_key.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
_L.vgen_solana_keypair_base58.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
_L.vgen_solana_decode.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
_L.vgen_onion_encode.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
_L.vgen_onion_decode.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
_L.vgen_onion_expand.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
_L.vgen_onion_base.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
_L.vgen_dispatch_onion.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint64]
_L.vgen_create2_address.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
_L.vgen_create2_salt.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p]
_L.vgen_set_create2.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
_L.vgen_dispatch_create2.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64]
_L.vgen_score.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32)]
_L.vgen_set_score_min.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
_L.vgen_scan_create2.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                 ctypes.c_uint64, ctypes.POINTER(_ScanConfig), _PROGRESS, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32),
                                 ctypes.POINTER(_ScanResult)]
_L.vgen_create3_proxy_hash.argtypes = [ctypes.c_char_p]
_L.vgen_create3_address.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int32, ctypes.c_char_p, ctypes.c_char_p]
_L.vgen_set_create3.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int32]
_L.vgen_scan_create3.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                 ctypes.c_char_p, ctypes.c_int32, ctypes.c_uint64, ctypes.POINTER(_ScanConfig), _PROGRESS, ctypes.c_void_p,
                                 ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_ScanResult)]
_L.vgen_set_base_point.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
_L.vgen_get_base_point.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int32)]
_L.vgen_split_dropped.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
_L.vgen_split_derive.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t]
_L.vgen_split_combine.argtypes = [ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32)]
_L.vgen_device_name.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
_L.vgen_scan.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(_ScanConfig), _PROGRESS, ctypes.c_void_p,
                         ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_ScanResult)]
_L.vgen_scan_multi.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_char_p,
                               ctypes.POINTER(_ScanConfig), _PROGRESS, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32),
                               ctypes.POINTER(_ScanResult)]
_L.vgen_filter_compile_list.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]
_L.vgen_filter_pattern_count.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
_L.vgen_filter_pattern.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t]
_L.vgen_filter_which.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32,
                                 ctypes.POINTER(ctypes.c_uint32)]
_L.vgen_scan_list.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                              ctypes.POINTER(_ScanConfig), _PROGRESS, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32),
                              ctypes.POINTER(_ScanResult)]
_L.vgen_scan_result_free.argtypes = [ctypes.POINTER(_ScanResult)]
_L.vgen_scan_result_free.restype = None


def _key(k):
    return k.to_bytes(32, "big") if isinstance(k, int) else bytes(k)


def _check(rc, ctx=None):
    if rc < 0:
        msg = _L.vgen_last_error(ctx)
        raise VgenError(rc, msg.decode() if msg else "")
    return rc


def abi_version():
    return _L.vgen_abi_version()


def device_count():
    n = ctypes.c_int(0)
    _check(_L.vgen_device_count(ctypes.byref(n)))
    return n.value


def device_name(device=0):
    buf = ctypes.create_string_buffer(256)
    _check(_L.vgen_device_name(device, buf, 256))
    return buf.value.decode()


def address_from_payload(fmt, payload):
    out = ctypes.create_string_buffer(128)
    _check(_L.vgen_address_from_payload(int(fmt), bytes(payload), out, 128))
    return out.value.decode()


def key_to_wif(fmt, key):
    out = ctypes.create_string_buffer(128)
    _check(_L.vgen_key_to_wif(int(fmt), _key(key), out, 128))
    return out.value.decode()


def key_add(key, amount):
    """increment_key (src/gpu.rs:951-968): None on overflow or an invalid scalar."""
    out = ctypes.create_string_buffer(32)
    rc = _L.vgen_key_add(_key(key), amount, out)
    return None if rc == E_RANGE else int.from_bytes(out.raw, "big")


def random_key(seed, stream, index):
    """vgen_random_key: candidate `index` of stream `stream` under `seed` of the counter-based scalar stream
    (vgen_dispatch_random); None when that draw is not a valid scalar.  seed: an integer < 2^64 (vgen_random_key) or the 24
    seed bytes themselves (vgen_random_key_seed)."""
    out = ctypes.create_string_buffer(32)
    if isinstance(seed, (bytes, bytearray)):
        assert len(seed) == 24
        rc = _L.vgen_random_key_seed(bytes(seed), stream, index, out)
    else:
        rc = _L.vgen_random_key(seed, stream, index, out)
    if rc == -7:
        return None
    _check(rc)
    return int.from_bytes(out.raw, "big")


def key_variant(key, variant):
    """vgen_key_variant: the key an endomorphism context tests as `variant` of base key `key`."""
    out = ctypes.create_string_buffer(32)
    _check(_L.vgen_key_variant(_key(key), variant, out))
    return int.from_bytes(out.raw, "big")


def _pubkey(pub) -> bytes:
    """A SEC1 public key as bytes: 33 / 65 bytes, or their hex string (an optional 0x in front)."""
    if isinstance(pub, str):
        pub = bytes.fromhex(pub[2:] if pub[:2] in ("0x", "0X") else pub)
    return bytes(pub)


def split_derive(fmt, pub, partial, variant: int = 0) -> Optional[str]:
    """vgen_split_derive: the address of image `variant` of the point P + partial * G, for the requester's public key `pub` (SEC1,
    33 or 65 bytes or hex) - what a split-key search reports for the partial key `partial`.  None when the sum is the point at
    infinity or `partial` is not below n; VgenError for a bad public key, variant or format."""
    pub, out = _pubkey(pub), ctypes.create_string_buffer(128)
    rc = _L.vgen_split_derive(int(fmt), pub, len(pub), _key(partial), variant, out, 128)
    if rc == E_RANGE:
        return None
    if rc < 0:
        raise VgenError(rc, "vgen_split_derive: bad public key, variant or format")
    return out.value.decode()


def split_combine(fmt, secret, partial, address: str):
    """vgen_split_combine, the requester's side of a split-key search: (final key, variant) with final key = the image `variant` of
    (secret + partial) mod n whose address is `address`.  VgenError when no image of the sum has that address (a wrong secret, a
    wrong partial key or a wrong address) or the sum is no key."""
    out, v = ctypes.create_string_buffer(32), ctypes.c_uint32()
    rc = _L.vgen_split_combine(int(fmt), _key(secret), _key(partial), address.encode(), out, ctypes.byref(v))
    if rc < 0:
        raise VgenError(rc, "vgen_split_combine: no image of secret + partial has this address" if rc == -1 else "vgen_split_combine: secret + partial is not a key, or the format has none")
    return int.from_bytes(out.raw, "big"), v.value


def nostr_encode(kind: str, data: bytes) -> str:
    """vgen_nostr_encode: NIP-19 Bech32 of 32 bytes; kind "npub" (an x-only public key) or "nsec" (a secret key)."""
    out = ctypes.create_string_buffer(128)
    _check(_L.vgen_nostr_encode({"npub": 0, "nsec": 1}[kind], bytes(data), out, 128))
    return out.value.decode()


def nostr_decode(text: str):
    """vgen_nostr_decode (strict) -> (kind, 32 bytes), or None when `text` is no npub / nsec string."""
    kind, out = ctypes.c_uint32(), ctypes.create_string_buffer(32)
    if _L.vgen_nostr_decode(text.encode(), ctypes.byref(kind), out) != 0:
        return None
    return ("npub", "nsec")[kind.value], out.raw


def npub_from_key(key) -> str:
    """The Nostr public key npub1... of a secret key (an integer or 32 big-endian bytes): Bech32 of x(key * G)."""
    return derive(FORMAT_NOSTR, key).address


def nsec_from_key(key) -> str:
    """The NIP-19 rendering nsec1... of a secret key, as it is (no parity normalisation)."""
    return key_to_wif(FORMAT_NOSTR, key)


def _seed32(seed) -> bytes:
    seed = bytes.fromhex(seed) if isinstance(seed, str) else bytes(seed)
    if len(seed) != 32:
        raise ValueError("an Ed25519 seed is 32 bytes")
    return seed


def solana_seed(seed, stream: int, index: int) -> bytes:
    """vgen_solana_seed: the 32-byte Ed25519 seed a Solana runner's dispatch_random tests as candidate `index` of stream `stream`.
    seed: an integer < 2^64 (standing for its 8 little-endian bytes and sixteen zero bytes) or the 24 seed bytes."""
    if not isinstance(seed, (bytes, bytearray)):
        seed = int(seed).to_bytes(8, "little") + bytes(16)
    assert len(seed) == 24
    out = ctypes.create_string_buffer(32)
    _check(_L.vgen_solana_seed(bytes(seed), stream, index, out))
    return out.raw


def solana_public_key(seed) -> bytes:
    """vgen_solana_public_key: the Ed25519 public key (RFC 8032) of a 32-byte seed - the 32 bytes of the address."""
    out = ctypes.create_string_buffer(32)
    _check(_L.vgen_solana_public_key(_seed32(seed), out))
    return out.raw


def solana_address(seed) -> str:
    """The Solana address of a seed: Base58 of its public key."""
    return address_from_payload(FORMAT_SOLANA, solana_public_key(seed))


def solana_keypair_base58(seed) -> str:
    """vgen_solana_keypair_base58: Base58 of seed || public key, the string wallets import as a private key."""
    out = ctypes.create_string_buffer(96)
    _check(_L.vgen_solana_keypair_base58(_seed32(seed), out, 96))
    return out.value.decode()


def solana_decode(address: str) -> Optional[bytes]:
    """vgen_solana_decode (strict) -> the 32 bytes, or None when `address` is not Base58 of exactly 32 bytes."""
    out = ctypes.create_string_buffer(32)
    if _L.vgen_solana_decode(address.encode(), out) != 0:
        return None
    return out.raw


def _scalar_le(scalar) -> bytes:
    if isinstance(scalar, int):
        return scalar.to_bytes(32, "little")
    scalar = bytes.fromhex(scalar) if isinstance(scalar, str) else bytes(scalar)
    if len(scalar) != 32:
        raise ValueError("an Ed25519 scalar is 32 little-endian bytes")
    return scalar


def onion_address(pub) -> str:
    """vgen_onion_encode: the 56-character Tor v3 address (without ".onion") of a 32-byte Ed25519 public key."""
    pub = bytes.fromhex(pub) if isinstance(pub, str) else bytes(pub)
    if len(pub) != 32:
        raise ValueError("an Ed25519 public key is 32 bytes")
    out = ctypes.create_string_buffer(64)
    _check(_L.vgen_onion_encode(pub, out, 64))
    return out.value.decode()


def onion_decode(address: str) -> Optional[bytes]:
    """vgen_onion_decode (strict) -> the 32 bytes of the public key, or None: wrong length, upper or mixed case, a character outside
    a-z2-7, a version other than 3 or a bad checksum.  A trailing ".onion" is accepted."""
    out = ctypes.create_string_buffer(32)
    if _L.vgen_onion_decode(address.encode(), out) != 0:
        return None
    return out.raw


def onion_expand(scalar) -> bytes:
    """vgen_onion_expand: the 64 bytes of Tor's expanded secret key - the scalar (an int, or its 32 little-endian bytes) and a nonce
    key derived from it."""
    out = ctypes.create_string_buffer(64)
    _check(_L.vgen_onion_expand(_scalar_le(scalar), out))
    return out.raw


def onion_base(seed, stream: int) -> bytes:
    """vgen_onion_base: the base scalar (32 little-endian bytes) an onion scan's shard `stream` walks from.
    seed: an integer < 2^64 (standing for its 8 little-endian bytes and sixteen zero bytes) or the 24 seed bytes."""
    if not isinstance(seed, (bytes, bytearray)):
        seed = int(seed).to_bytes(8, "little") + bytes(16)
    assert len(seed) == 24
    out = ctypes.create_string_buffer(32)
    _check(_L.vgen_onion_base(bytes(seed), stream, out))
    return out.raw


def contract_address(deployer, nonce=0) -> bytes:
    """vgen_contract_address: the 20 bytes of the contract the account `deployer` (20 bytes, or a 0x-hex string) creates with the
    transaction of the given nonce: keccak256(rlp([deployer, nonce]))[12:]."""
    if isinstance(deployer, str):
        deployer = bytes.fromhex(deployer[2:] if deployer[:2] in ("0x", "0X") else deployer)
    if len(deployer) != 20 or not 0 <= nonce < 1 << 64:
        raise ValueError("deployer is 20 bytes, nonce < 2^64")
    out = ctypes.create_string_buffer(20)
    _check(_L.vgen_contract_address(bytes(deployer), nonce, out))
    return out.raw


def _hexbytes(v, n, what):
    if isinstance(v, str):
        v = bytes.fromhex(v[2:] if v[:2] in ("0x", "0X") else v)
    v = bytes(v)
    if len(v) != n:
        raise ValueError("%s is %d bytes" % (what, n))
    return v


def keccak256(data) -> bytes:
    """vgen_keccak256: Keccak-256 (Ethereum's, pre-SHA-3 padding) of any number of bytes."""
    data = bytes(data)
    out = ctypes.create_string_buffer(32)
    _check(_L.vgen_keccak256(data, len(data), out))
    return out.raw


def create2_address(deployer, salt, init_code_hash) -> bytes:
    """vgen_create2_address: keccak256(0xff || deployer || salt || init_code_hash)[12:] (EIP-1014); bytes or 0x-hex strings."""
    out = ctypes.create_string_buffer(20)
    _check(_L.vgen_create2_address(_hexbytes(deployer, 20, "deployer"), _hexbytes(salt, 32, "salt"), _hexbytes(init_code_hash, 32, "init_code_hash"), out))
    return out.raw


class Create2Job:
    """What a CREATE2 salt search is about: the factory `deployer` that executes CREATE2, the hash of the init code (or the init code
    itself) and the caller's part of the salt, `salt_prefix` (up to 24 bytes, left-aligned, zero padded).  Candidate `counter` is the
    salt salt_prefix || counter as 8 big-endian bytes."""

    def __init__(self, deployer, init_code_hash=None, init_code=None, salt_prefix=b""):
        if (init_code_hash is None) == (init_code is None):
            raise ValueError("give exactly one of init_code_hash and init_code")
        self.deployer = _hexbytes(deployer, 20, "deployer")
        self.init_code_hash = keccak256(init_code) if init_code is not None else _hexbytes(init_code_hash, 32, "init_code_hash")
        if isinstance(salt_prefix, str):
            salt_prefix = bytes.fromhex(salt_prefix[2:] if salt_prefix[:2] in ("0x", "0X") else salt_prefix)
        if len(salt_prefix) > 24:
            raise ValueError("salt_prefix is at most 24 bytes")
        self.salt_prefix = bytes(salt_prefix).ljust(24, b"\0")

    def salt(self, counter: int) -> bytes:
        """vgen_create2_salt."""
        out = ctypes.create_string_buffer(32)
        _check(_L.vgen_create2_salt(self.salt_prefix, counter, out))
        return out.raw

    def address(self, counter: int) -> bytes:
        return create2_address(self.deployer, self.salt(counter), self.init_code_hash)


def _guard_args(guard):
    """(pointer, length) of an optional guard for the C ABI: None is no guard (-1), b"" the guard of length 0."""
    if guard is None:
        return None, -1
    if isinstance(guard, str):
        guard = bytes.fromhex(guard[2:] if guard[:2] in ("0x", "0X") else guard)
    guard = bytes(guard)
    if len(guard) > 64:
        raise ValueError("guard is at most 64 bytes")
    return guard, len(guard)


def create3_proxy_hash() -> bytes:
    """vgen_create3_proxy_hash: keccak256 of the 16-byte proxy that Solmate / Solady CREATE3 and CreateX deploy."""
    out = ctypes.create_string_buffer(32)
    _check(_L.vgen_create3_proxy_hash(out))
    return out.raw


def create3_address(factory, salt, proxy_init_code_hash=None, guard=None, with_proxy=False):
    """vgen_create3_address: the address of the contract a CREATE3 factory deploys for the raw `salt`; guard=None is no guard, bytes
    (0 to 64 of them) are hashed in front of the salt.  with_proxy=True returns (proxy, contract)."""
    g, n = _guard_args(guard)
    h = create3_proxy_hash() if proxy_init_code_hash is None else _hexbytes(proxy_init_code_hash, 32, "proxy_init_code_hash")
    proxy, out = ctypes.create_string_buffer(20), ctypes.create_string_buffer(20)
    _check(_L.vgen_create3_address(_hexbytes(factory, 20, "factory"), _hexbytes(salt, 32, "salt"), h, g, n, proxy, out))
    return (proxy.raw, out.raw) if with_proxy else out.raw


class Create3Job:
    """What a CREATE3 salt search is about: the `factory`, the hash of the proxy it deploys (None: the usual proxy's), the caller's
    part of the raw salt (up to 24 bytes, left-aligned, zero padded) and the guard the factory hashes in front of the salt
    (None: the factory uses the raw salt; b"": keccak256(salt); e.g. the 20 bytes of msg.sender for ZeframLou's factory).
    Candidate `counter` is the raw salt salt_prefix || counter as 8 big-endian bytes: what the factory is called with."""

    def __init__(self, factory, proxy_init_code_hash=None, salt_prefix=b"", guard=None):
        self.factory = _hexbytes(factory, 20, "factory")
        self.proxy_init_code_hash = create3_proxy_hash() if proxy_init_code_hash is None else _hexbytes(proxy_init_code_hash, 32, "proxy_init_code_hash")
        if isinstance(salt_prefix, str):
            salt_prefix = bytes.fromhex(salt_prefix[2:] if salt_prefix[:2] in ("0x", "0X") else salt_prefix)
        if len(salt_prefix) > 24:
            raise ValueError("salt_prefix is at most 24 bytes")
        self.salt_prefix = bytes(salt_prefix).ljust(24, b"\0")
        self.guard, self.guard_len = _guard_args(guard)

    def salt(self, counter: int) -> bytes:
        """The raw salt (vgen_create2_salt)."""
        out = ctypes.create_string_buffer(32)
        _check(_L.vgen_create2_salt(self.salt_prefix, counter, out))
        return out.raw

    def guarded_salt(self, counter: int) -> bytes:
        """The salt the proxy is deployed under: keccak256(guard || salt), or the raw salt without a guard."""
        return self.salt(counter) if self.guard is None else keccak256(self.guard + self.salt(counter))

    def proxy(self, counter: int) -> bytes:
        return create3_address(self.factory, self.salt(counter), self.proxy_init_code_hash, self.guard, with_proxy=True)[0]

    def address(self, counter: int) -> bytes:
        return create3_address(self.factory, self.salt(counter), self.proxy_init_code_hash, self.guard)


@dataclass
class GeneratedAddress:
    address: str
    wif: str
    hex: str
    format: AddressFormat


def derive(fmt, key) -> Optional[GeneratedAddress]:
    """AddressGenerator::generate on the host (src/address.rs:92-151); None for an invalid key."""
    a, w = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128)
    rc = _L.vgen_derive(int(fmt), _key(key), a, 128, w, 128)
    if rc == E_RANGE:
        return None
    _check(rc)
    return GeneratedAddress(a.value.decode(), w.value.decode(), _key(key).hex(), _fmt(fmt))


class Pattern:
    """Pattern::new / matches (src/pattern.rs:21-45) plus the device prefilter derived for `fmt`."""

    def __init__(self, pattern: str, case_insensitive: bool = False, fmt: AddressFormat = AddressFormat.P2pkh):
        self.original, self.case_insensitive, self.format = pattern, case_insensitive, _fmt(fmt)
        h = ctypes.c_void_p()
        _check(_L.vgen_filter_compile(pattern.encode(), int(case_insensitive), int(fmt), ctypes.byref(h)))
        self._h = h

    def matches(self, address: str) -> bool:
        return _L.vgen_filter_matches(self._h, address.encode()) == 1

    @property
    def device_kind(self) -> int:
        return _L.vgen_filter_device_kind(self._h)

    @property
    def dfa_bytes(self) -> int:
        """vgen_filter_dfa_bytes: LDS bytes of the on-device automaton (device_kind 4), else 0."""
        return _L.vgen_filter_dfa_bytes(self._h)

    def validate_charset(self, fmt: Optional[AddressFormat] = None) -> List[str]:
        """Pattern::validate_charset (src/pattern.rs:49-177): characters that can never occur in `fmt` addresses."""
        fmt = self.format if fmt is None else fmt
        buf, n = ctypes.create_string_buffer(260), ctypes.c_size_t()
        _check(_L.vgen_pattern_invalid_chars(self.original.encode(), int(self.case_insensitive), int(fmt), buf, 260,
                                             ctypes.byref(n)))
        return list(buf.value.decode())

    def estimate_difficulty(self, fmt: Optional[AddressFormat] = None) -> int:
        """Pattern::estimate_difficulty (src/pattern.rs:183-253): 1 in N addresses is expected to match."""
        fmt = self.format if fmt is None else fmt
        d = ctypes.c_uint64()
        _check(_L.vgen_pattern_difficulty(self.original.encode(), int(self.case_insensitive), int(fmt), ctypes.byref(d)))
        return d.value

    def is_case_insensitive(self) -> bool:
        return self.case_insensitive

    def score(self, address: str) -> int:
        """vgen_score: the score of `address` under a score specification ("score:zero-bytes>=2&leading:0>=4": the value of the
        first term's metric).  VgenError for any other pattern and for a string that is no address of the format."""
        v = ctypes.c_uint32()
        rc = _L.vgen_score(self._h, address.encode(), ctypes.byref(v))
        if rc < 0:
            raise VgenError(rc, "vgen_score: not a score specification, or not an address of its format")
        return v.value

    def __del__(self):
        if getattr(self, "_h", None):
            _L.vgen_filter_free(self._h)
            self._h = None


def score(filter_or_spec, address: str, fmt: AddressFormat = AddressFormat.Ethereum) -> int:
    """The score of `address` under a score specification: a Pattern compiled from one, or the specification's text (compiled for
    `fmt`, one of the three hex formats)."""
    p = filter_or_spec if isinstance(filter_or_spec, Pattern) else Pattern(filter_or_spec, fmt=fmt)
    return p.score(address)


class PatternList:
    """A list of patterns matched in one scan (vgen_filter_compile_list): one pattern per line of `patterns` (or an
    iterable of lines), start-anchored prefixes only; device kind 5.  Raises VgenError with "line N: reason" otherwise."""

    def __init__(self, patterns, case_insensitive: bool = False, fmt: AddressFormat = AddressFormat.P2pkh):
        text = patterns if isinstance(patterns, str) else "\n".join(patterns)
        self.case_insensitive, self.format = case_insensitive, _fmt(fmt)
        h = ctypes.c_void_p()
        _check(_L.vgen_filter_compile_list(text.encode(), int(case_insensitive), int(fmt), ctypes.byref(h)))
        self._h = h
        n = ctypes.c_uint32()
        _check(_L.vgen_filter_pattern_count(h, ctypes.byref(n)))
        self._n = n.value

    def __len__(self) -> int:
        return self._n

    def pattern(self, index: int) -> str:
        """Text of pattern `index` (what the command line prints in a result's `pattern` field)."""
        buf = ctypes.create_string_buffer(4096)
        rc = _L.vgen_filter_pattern(self._h, index, buf, 4096)
        _check(rc)
        return buf.value.decode()

    def which(self, address: str) -> List[int]:
        """vgen_filter_which: every pattern index the address satisfies, ascending."""
        cap = 64
        while True:
            arr, n = (ctypes.c_uint32 * cap)(), ctypes.c_uint32()
            _check(_L.vgen_filter_which(self._h, address.encode(), arr, cap, ctypes.byref(n)))
            if n.value <= cap:
                return list(arr[:n.value])
            cap = n.value

    def matches(self, address: str) -> bool:
        return _L.vgen_filter_matches(self._h, address.encode()) == 1

    @property
    def device_kind(self) -> int:
        return _L.vgen_filter_device_kind(self._h)

    def __del__(self):
        if getattr(self, "_h", None):
            _L.vgen_filter_free(self._h)
            self._h = None


@dataclass
class ListMatch(GeneratedAddress):
    """A result of scan_list: the address and the lowest index of the patterns it satisfies."""
    pattern_index: int = -1


@dataclass
class ProviderResult:
    """ProviderResult (src/provider.rs:6-10)."""
    address: str
    format: AddressFormat
    key_range: Optional[tuple] = None


def provider_resolve(pattern: str, table_path: Optional[str] = None) -> Optional[ProviderResult]:
    """provider::resolve (src/provider.rs:12-52): None when `pattern` is an ordinary regex."""
    addr, fmt, has = ctypes.create_string_buffer(128), ctypes.c_uint32(), ctypes.c_int32()
    lo, hi = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
    rc = _L.vgen_provider_resolve(pattern.encode(), os.fsencode(table_path) if table_path else None, addr, 128,
                                  ctypes.byref(fmt), ctypes.byref(has), lo, hi)
    if rc == 0:
        return None
    _check(rc if rc < 0 else 0)
    rng = (int.from_bytes(lo.raw, "big"), int.from_bytes(hi.raw, "big")) if has.value else None
    return ProviderResult(addr.value.decode(), AddressFormat(fmt.value), rng)


def build_pattern(result: ProviderResult, prefix_length: int) -> str:
    """provider::build_pattern (src/provider.rs:54-58)."""
    if prefix_length < 1:
        raise ValueError("--prefix-length must be at least 1 for provider patterns")   # lib.rs:570-572
    out = ctypes.create_string_buffer(300)
    _check(_L.vgen_provider_build_pattern(result.address.encode(), prefix_length, out, 300))
    return out.value.decode()


def build_exact_pattern(result: ProviderResult) -> str:
    """provider::build_exact_pattern (src/provider.rs:60-62)."""
    out = ctypes.create_string_buffer(300)
    _check(_L.vgen_provider_build_pattern(result.address.encode(), 0, out, 300))
    return out.value.decode()


@dataclass
class ScanConfig:
    """src/scanner.rs:17-46 (fields the GPU path reads) + the build-side seed / shard additions."""
    format: AddressFormat = AddressFormat.P2pkh
    count: int = 1
    gpu_batch_size: Optional[int] = None
    start: Optional[int] = None
    end: Optional[int] = None
    case_insensitive: bool = False
    seed: int = 0
    shard: int = 0
    n_shards: int = 1
    max_batches: int = 0
    checkpoint_path: Optional[str] = None      # resumable scans (vgen_scan_config.checkpoint_path)
    checkpoint_interval_ms: int = 0
    random_keys: bool = False       # VGEN_SCAN_RANDOM_KEYS: an independent random key per candidate (scanner.rs:118-169's shape)
    table_bits_max: int = 0         # widest generator table the scan may move the context to (0 = the context's memory policy decides)
    best: bool = False              # VGEN_SCAN_BEST (score specifications): report only results that beat every score reported before


@dataclass
class ScanResult:
    matches: List[GeneratedAddress] = field(default_factory=list)
    operations: int = 0
    elapsed_secs: float = 0.0
    resumed_operations: int = 0     # operations recorded in the checkpoint this call resumed from
    complete: bool = False          # the key range ran out
    failed_shards: int = 0          # contexts that failed during the scan (their stripes were taken over by the others)

    def rate(self) -> float:   # src/scanner.rs:61-67
        return self.operations / self.elapsed_secs if self.elapsed_secs > 0 else 0.0


class GpuRunner:
    """GpuRunner (src/gpu.rs:116-131): one device, `frames` dispatches in flight."""

    def __init__(self, batch_size: int = 1 << 20, fmt: AddressFormat = AddressFormat.P2pkh, device: int = 0,
                 frames: int = 2, match_cap: int = 4096, timing: bool = True, endo: bool = False, table_bits: int = 0,
                 device_mem_budget_bytes: int = 0):
        # timing: VGEN_FLAG_TIMING — events around every dispatch so that kernel_ms() / dispatch_ms() work
        # endo: VGEN_FLAG_ENDO — six keys per curve point (vanity searches on compressed-key formats; three for Nostr's x-only keys)
        # table_bits / device_mem_budget_bytes: the generator-table width and the device-memory bound of this context (0 = automatic)
        p = _Params(ctypes.sizeof(_Params), device, batch_size, int(fmt), frames, match_cap, (1 if timing else 0) | (2 if endo else 0),
                    table_bits, device_mem_budget_bytes)
        h = ctypes.c_void_p()
        _check(_L.vgen_create(ctypes.byref(p), ctypes.byref(h)))
        self._h = h
        b, f, m = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _L.vgen_get_info(h, ctypes.byref(b), ctypes.byref(f), ctypes.byref(m))
        self.batch_size, self.frames, self.match_cap, self.format = b.value, f.value, m.value, _fmt(fmt)
        self.payload_bytes = 32 if int(self.format) in (int(AddressFormat.P2tr), FORMAT_NOSTR, FORMAT_SOLANA, FORMAT_ONION) else 20
        self._pattern = None

    def topology(self) -> dict:
        """vgen_get_topology: streams of the context (one per frame), the HIP hardware-queue limit per stream priority
        level, the number of levels, and whether every stream owns a queue."""
        a, q, l, o = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int32()
        _check(_L.vgen_get_topology(self._h, ctypes.byref(a), ctypes.byref(q), ctypes.byref(l), ctypes.byref(o)), self._h)
        return {"streams": a.value, "hw_queues": q.value, "priority_levels": l.value, "oversubscribed": bool(o.value)}

    def dump_view(self, frame: int) -> bytes:
        """vgen_dump_view: the frame's payloads from the pinned buffer its dump-mode dispatch copied itself into."""
        ptr, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(_L.vgen_dump_view(self._h, frame, ctypes.byref(ptr), ctypes.byref(n)), self._h)
        return ctypes.string_at(ptr.value, n.value)

    def close(self):
        if getattr(self, "_h", None):
            _L.vgen_destroy(self._h)
            self._h = None

    __del__ = close

    def set_filter(self, pattern):
        """A Pattern, a PatternList (candidates: a superset the host confirms with which()), or None for dump mode."""
        _check(_L.vgen_set_filter(self._h, pattern._h if pattern else None), self._h)
        self._pattern = pattern

    def dispatch(self, start_key, frame: int):
        _check(_L.vgen_dispatch(self._h, frame, _key(start_key)), self._h)

    def dispatch_keys(self, keys, frame: int):
        """vgen_dispatch_keys: arbitrary scalars (ints, 32-byte strings, or one n*32-byte blob), full k*G per key."""
        if isinstance(keys, (bytes, bytearray)):     # already n * 32 big-endian bytes
            blob, n = bytes(keys), len(keys) // 32
        else:
            blob, n = b"".join(_key(k) for k in keys), len(keys)
        self._n_keys = n
        _check(_L.vgen_dispatch_keys(self._h, frame, blob, n), self._h)

    def set_base(self, pub):
        """vgen_set_base_point: split-key search - every dispatch of this runner tests P + k * G for the requester's public key P
        (SEC1, 33 or 65 bytes or hex) and scans report the partial keys k; None clears it.  Only while nothing is in flight."""
        pub = None if pub is None else _pubkey(pub)
        _check(_L.vgen_set_base_point(self._h, pub, len(pub) if pub else 0), self._h)

    @property
    def base(self) -> Optional[bytes]:
        """vgen_get_base_point: the installed base point as 65 uncompressed bytes, or None."""
        out, is_set = ctypes.create_string_buffer(65), ctypes.c_int32()
        _check(_L.vgen_get_base_point(self._h, out, ctypes.byref(is_set)), self._h)
        return out.raw if is_set.value else None

    @property
    def split_dropped(self) -> int:
        """vgen_split_dropped: candidates of this runner's split-key scans that the host's re-derivation refused."""
        n = ctypes.c_uint64()
        _check(_L.vgen_split_dropped(self._h, ctypes.byref(n)), self._h)
        return n.value

    def set_create2(self, job: "Create2Job"):
        """vgen_set_create2: the job of an EthereumCreate2 runner."""
        _check(_L.vgen_set_create2(self._h, job.deployer, job.init_code_hash, job.salt_prefix), self._h)

    def set_score_min(self, minimum: int):
        """vgen_set_score_min: the first term's threshold of the installed score filter, for dispatches enqueued from now on."""
        _check(_L.vgen_set_score_min(self._h, minimum), self._h)

    def set_create3(self, job: "Create3Job"):
        """vgen_set_create3: a CREATE3 job on an EthereumCreate2 runner; dispatch_create2 then tests its salts."""
        _check(_L.vgen_set_create3(self._h, job.factory, job.proxy_init_code_hash, job.salt_prefix, job.guard, job.guard_len), self._h)

    def dispatch_onion(self, base_scalar, first_index: int, frame: int):
        """vgen_dispatch_onion: candidate i has the Ed25519 scalar base + 8 * (first_index + i); base_scalar an int or its 32
        little-endian bytes, a multiple of 8.  Results as for dispatch()."""
        self._n_keys = self.batch_size
        _check(_L.vgen_dispatch_onion(self._h, frame, _scalar_le(base_scalar), first_index), self._h)

    def dispatch_create2(self, first_counter: int, frame: int):
        """vgen_dispatch_create2: salts first_counter .. first_counter + batch_size - 1 of the job; results as for dispatch()."""
        _check(_L.vgen_dispatch_create2(self._h, frame, first_counter), self._h)

    def fail_after(self, dispatches: int):
        """vgen_debug_fail_after: fault injection — dispatches fail with VGEN_E_HIP once `dispatches` more were accepted.
        Exists only in the test build of the library (tests/conftest.py: hooks_api)."""
        if not hasattr(_L, "vgen_debug_fail_after"):
            raise RuntimeError("fault injection is not part of libvgen_hip.so: load tests/native/libvgen_hip_hooks.so (tests/conftest.py: hooks_api)")
        _check(_L.vgen_debug_fail_after(self._h, dispatches), self._h)

    def resources(self):
        """vgen_get_resources -> dict(dump_frames, table_bits, table_bits_wanted, note)."""
        d, b, w = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        note = ctypes.create_string_buffer(256)
        _check(_L.vgen_get_resources(self._h, ctypes.byref(d), ctypes.byref(b), ctypes.byref(w), note, 256), self._h)
        return {"dump_frames": d.value, "table_bits": b.value, "table_bits_wanted": w.value, "note": note.value.decode()}

    def memory(self):
        """vgen_get_memory -> dict of the context's device / pinned host bytes, its budget and the device's free / total bytes."""
        m = _MemoryInfo()
        m.struct_size = ctypes.sizeof(_MemoryInfo)
        _check(_L.vgen_get_memory(self._h, ctypes.byref(m)), self._h)
        return {k: getattr(m, k) for k, _ in _MemoryInfo._fields_ if k != "struct_size"}

    def dispatch_random(self, seed, stream: int, first_index: int, frame: int):
        """vgen_dispatch_random: batch_size independent random keys drawn on the device from the counter-based stream.
        seed: an integer < 2^64 or the 24 seed bytes (vgen_dispatch_random_seed)."""
        self._n_keys = self.batch_size
        if isinstance(seed, (bytes, bytearray)):
            assert len(seed) == 24
            _check(_L.vgen_dispatch_random_seed(self._h, frame, bytes(seed), stream, first_index), self._h)
        else:
            _check(_L.vgen_dispatch_random(self._h, frame, seed, stream, first_index), self._h)

    def await_result(self, frame: int):
        """Filter mode: (list of (index, payload20), n_found, keys_tested).  Dump mode: (bytes, 0, keys_tested)."""
        recs = (_Match * self.match_cap)()
        n, tested = ctypes.c_uint32(), ctypes.c_uint64()
        _check(_L.vgen_wait(self._h, frame, recs, self.match_cap, ctypes.byref(n), ctypes.byref(tested)), self._h)
        if self._pattern is None:
            return self.dump_view(frame), 0, tested.value
        k = min(n.value, self.match_cap)
        return [(recs[i].index, bytes(recs[i].payload)[:self.payload_bytes]) for i in range(k)], n.value, tested.value

    def wait(self, frame: int):
        """vgen_wait without fetching anything (benchmark loop)."""
        n, tested = ctypes.c_uint32(), ctypes.c_uint64()
        _check(_L.vgen_wait(self._h, frame, None, 0, ctypes.byref(n), ctypes.byref(tested)), self._h)
        return n.value, tested.value

    def clock_probe_start(self, duration_ms: int):
        """Samples the shader clock for duration_ms on a side stream (vgen_clock_probe_start)."""
        _check(_L.vgen_clock_probe_start(self._h, duration_ms), self._h)

    def clock_probe_read(self) -> float:
        mhz = ctypes.c_double()
        _check(_L.vgen_clock_probe_read(self._h, ctypes.byref(mhz)), self._h)
        return mhz.value

    def kernel_ms(self, frame: int) -> float:
        """HIP-event duration of the dominant kernel (seq_bwd_kernel) of the frame's last dispatch."""
        ms = ctypes.c_float()
        _check(_L.vgen_frame_kernel_ms(self._h, frame, ctypes.byref(ms)), self._h)
        return ms.value

    def frame_clock(self, frame: int):
        """vgen_frame_clock: (shader-clock cycles, 100 MHz ticks) sampled by the frame's last seq_bwd launch."""
        c, t = ctypes.c_uint32(), ctypes.c_uint32()
        _check(_L.vgen_frame_clock(self._h, frame, ctypes.byref(c), ctypes.byref(t)), self._h)
        return c.value, t.value

    def dispatch_ms(self, frame: int) -> float:
        """HIP-event duration of the whole last dispatch (seq_fwd incl. the root inversions + seq_bwd)."""
        ms = ctypes.c_float()
        _check(_L.vgen_frame_dispatch_ms(self._h, frame, ctypes.byref(ms)), self._h)
        return ms.value


def _scan_config(config: ScanConfig) -> _ScanConfig:
    c = _ScanConfig()
    c.struct_size = ctypes.sizeof(_ScanConfig)
    c.format = int(config.format)
    c.count = config.count if config.count is not None else 2**64 - 1
    c.case_insensitive = int(config.case_insensitive)
    if config.start is not None:
        c.has_start = 1
        c.start = (ctypes.c_uint8 * 32)(*_key(config.start))
    if config.end is not None:
        c.has_end = 1
        c.end = (ctypes.c_uint8 * 32)(*_key(config.end))
    c.seed, c.shard, c.n_shards, c.max_batches = config.seed, config.shard, config.n_shards, config.max_batches
    if config.checkpoint_path:
        c.checkpoint_path = os.fsencode(config.checkpoint_path)
        c.checkpoint_interval_ms = config.checkpoint_interval_ms
    c.flags = (SCAN_RANDOM_KEYS if config.random_keys else 0) | (SCAN_BEST if config.best else 0)
    c.table_bits_max = config.table_bits_max
    return c


def scan_list(plist: PatternList, config: ScanConfig, runner, per_pattern: int = 1,
              progress_cb: Optional[Callable[[int], None]] = None, stop=None) -> ScanResult:
    """vgen_scan_list: one scan for every pattern of `plist` over one GpuRunner or a list of them.  config.format must be
    the list's; config.count (None = unbounded) caps the results in total, per_pattern (0 = unbounded) per pattern.
    The matches are ListMatch records in the scan's order, each with the lowest index of the patterns it satisfies."""
    runners = list(runner) if isinstance(runner, (list, tuple)) else [runner]
    c = _scan_config(config)
    res = _ScanResult()
    cb = _PROGRESS(lambda ops, _u: progress_cb(ops)) if progress_cb else ctypes.cast(None, _PROGRESS)
    stop_p = ctypes.byref(stop) if stop is not None else None
    arr = (ctypes.c_void_p * len(runners))(*[r._h for r in runners])
    rc = _L.vgen_scan_list(arr, len(runners), plist._h, per_pattern, ctypes.byref(c), cb, None, stop_p, ctypes.byref(res))
    out = ScanResult(operations=res.operations, elapsed_secs=res.elapsed_secs,
                     resumed_operations=res.resumed_operations, complete=bool(res.complete), failed_shards=res.failed_shards)
    for i in range(res.n_matches):
        g = res.matches[i]
        a = g.address.decode()
        w = plist.which(a)
        out.matches.append(ListMatch(a, g.wif.decode(), g.hex.decode(), _fmt(g.format), w[0] if w else -1))
    _L.vgen_scan_result_free(ctypes.byref(res))
    if rc < 0:
        msg = _L.vgen_last_error(runners[0]._h)
        err = VgenError(rc, msg.decode() if msg else "")
        err.partial = out
        raise err
    return out


def scan_gpu_with_runner(pattern: str, config: ScanConfig, runner,
                         progress_cb: Optional[Callable[[int], None]] = None, stop=None, force_multi: bool = False) -> ScanResult:
    """scan_gpu_with_runner (src/gpu.rs:920-926).  `stop` is an optional ctypes.c_int32 flag.
    `runner` may be a list of GpuRunners (one per GPU): the batches are then striped over them
    (vgen_scan_multi; force_multi: also for a list of one)."""
    runners = list(runner) if isinstance(runner, (list, tuple)) else [runner]
    runner = runners[0]
    c = _scan_config(config)
    res = _ScanResult()
    cb = _PROGRESS(lambda ops, _u: progress_cb(ops)) if progress_cb else ctypes.cast(None, _PROGRESS)
    stop_p = ctypes.byref(stop) if stop is not None else None
    if len(runners) == 1 and not force_multi:
        rc = _L.vgen_scan(runner._h, pattern.encode(), ctypes.byref(c), cb, None, stop_p, ctypes.byref(res))
    else:
        arr = (ctypes.c_void_p * len(runners))(*[r._h for r in runners])
        rc = _L.vgen_scan_multi(arr, len(runners), pattern.encode(), ctypes.byref(c), cb, None, stop_p, ctypes.byref(res))
    out = ScanResult(operations=res.operations, elapsed_secs=res.elapsed_secs,
                     resumed_operations=res.resumed_operations, complete=bool(res.complete), failed_shards=res.failed_shards)
    for i in range(res.n_matches):
        g = res.matches[i]
        out.matches.append(GeneratedAddress(g.address.decode(), g.wif.decode(), g.hex.decode(), _fmt(g.format)))
    _L.vgen_scan_result_free(ctypes.byref(res))
    if rc < 0:
        # a failing scan still hands over what its finished batches found (vgen_scan_result is filled, complete = 0)
        msg = _L.vgen_last_error(runner._h)
        err = VgenError(rc, msg.decode() if msg else "")
        err.partial = out
        raise err
    return out


def _salt_scan(call, pattern, config, runner, progress_cb, stop) -> ScanResult:
    runners = list(runner) if isinstance(runner, (list, tuple)) else [runner]
    c = _scan_config(config)
    res = _ScanResult()
    cb = _PROGRESS(lambda ops, _u: progress_cb(ops)) if progress_cb else ctypes.cast(None, _PROGRESS)
    stop_p = ctypes.byref(stop) if stop is not None else None
    arr = (ctypes.c_void_p * len(runners))(*[r._h for r in runners])
    rc = call(arr, len(runners), pattern.encode(), ctypes.byref(c), cb, stop_p, ctypes.byref(res))
    out = ScanResult(operations=res.operations, elapsed_secs=res.elapsed_secs, complete=bool(res.complete), failed_shards=res.failed_shards)
    for i in range(res.n_matches):
        g = res.matches[i]
        out.matches.append(GeneratedAddress(g.address.decode(), g.wif.decode(), g.hex.decode(), _fmt(g.format)))
    _L.vgen_scan_result_free(ctypes.byref(res))
    if rc < 0:
        msg = _L.vgen_last_error(runners[0]._h)
        err = VgenError(rc, msg.decode() if msg else "")
        err.partial = out
        raise err
    return out


def scan_create2(pattern: str, job: Create2Job, config: ScanConfig, runner, first_counter: int = 0,
                 progress_cb: Optional[Callable[[int], None]] = None, stop=None) -> ScanResult:
    """vgen_scan_create2: the salts of `job` from counter `first_counter` on, over one EthereumCreate2 GpuRunner or a list of them.
    In a match, `hex` (and `wif`) is "0x" + the 32-byte salt; the address exists only when job.deployer executes CREATE2 with that
    salt and the job's init code."""
    return _salt_scan(lambda arr, n, pat, c, cb, stop_p, res: _L.vgen_scan_create2(arr, n, pat, job.deployer, job.init_code_hash, job.salt_prefix,
                                                                                  first_counter, c, cb, None, stop_p, res),
                      pattern, config, runner, progress_cb, stop)


def scan_create3(pattern: str, job: Create3Job, config: ScanConfig, runner, first_counter: int = 0,
                 progress_cb: Optional[Callable[[int], None]] = None, stop=None) -> ScanResult:
    """vgen_scan_create3: the same search over a CREATE3 job.  In a match, `hex` (and `wif`) is "0x" + the 32-byte RAW salt, the one
    job.factory is called with; job.proxy(counter) and job.guarded_salt(counter) give the rest."""
    return _salt_scan(lambda arr, n, pat, c, cb, stop_p, res: _L.vgen_scan_create3(arr, n, pat, job.factory, job.proxy_init_code_hash, job.salt_prefix,
                                                                                  job.guard, job.guard_len, first_counter, c, cb, None, stop_p, res),
                      pattern, config, runner, progress_cb, stop)
