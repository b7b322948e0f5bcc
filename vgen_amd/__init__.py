"""vgen_amd — MI355X-native scan engine for the vanity-address hot path of oritwoen/vgen.

The product is vgen_amd/libvgen_hip.so (HIP kernels for gfx950 + host runtime behind the C ABI of
include/vgen_hip.h).  This package is the thin Python view of that ABI used by the tests and by
bench.py; names mirror the reference (src/address.rs, src/scanner.rs, src/pattern.rs, src/gpu.rs).
There is no CPU fallback: importing works anywhere, creating a GpuRunner needs an MI355X.
"""
from .api import (AddressFormat, FORMAT_NOSTR, FORMAT_SOLANA, FORMAT_ONION, onion_address, onion_decode, onion_expand, onion_base, solana_seed, solana_public_key, solana_address, solana_keypair_base58, solana_decode, Create2Job, Create3Job, create3_address, create3_proxy_hash, scan_create3, GeneratedAddress, GpuRunner, ListMatch, Pattern, PatternList, ScanConfig, ScanResult, VgenError,
                  abi_version, address_from_payload, contract_address, create2_address, derive, device_count, device_name, keccak256, key_add, key_variant,
                  key_to_wif, nostr_decode, nostr_encode, npub_from_key, nsec_from_key, random_key, scan_create2, score, split_combine, split_derive, library_path, scan_gpu_with_runner, scan_list, ProviderResult, provider_resolve, build_pattern, build_exact_pattern)

__all__ = ["AddressFormat", "FORMAT_NOSTR", "FORMAT_SOLANA", "FORMAT_ONION", "onion_address", "onion_decode", "onion_expand", "onion_base", "solana_seed", "solana_public_key", "solana_address", "solana_keypair_base58", "solana_decode", "Create2Job", "Create3Job", "create3_address", "create3_proxy_hash", "scan_create3", "GeneratedAddress", "GpuRunner", "ListMatch", "Pattern", "PatternList", "ScanConfig", "ScanResult", "VgenError",
           "abi_version", "address_from_payload", "contract_address", "create2_address", "keccak256", "scan_create2", "derive", "device_count", "device_name", "key_add", "key_variant",
           "key_to_wif", "nostr_decode", "nostr_encode", "npub_from_key", "nsec_from_key", "random_key", "score", "split_combine", "split_derive", "library_path", "scan_gpu_with_runner", "scan_list", "ProviderResult", "provider_resolve", "build_pattern",
           "build_exact_pattern"]
