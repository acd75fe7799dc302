// bmx_variants_product.inc -- the slots of the kernel table that libbmx.so contains (included by bmx_scan.hip inside the
// table's constructor; SLOT(i, entry) fills slot i).  Slot numbers are stable: tools/ and DESIGN.md refer to them.
// Everything here is parity-tested (tests/test_gpu_parity.py::PRODUCT_VARIANTS) and selectable with bmx_set_variant.
    SLOT(0, BMX_TILE_F(1024, 68, 2, 0)); // 0: PRODUCT -- 16 waves share a 68 KiB tile, nt DMA, byte-wise walker
    //    (the automatic choice for m < 4 and for dense small-alphabet results)
    SLOT(1, BMX_TILE_F(1024, 68, 2, 2)); // 1: PRODUCT -- same tile, skip-loop walker
    SLOT(2, BMX_TILE_W32(1024, 36, 2, 0, 2)); // 2: PRODUCT -- skip-loop walker, 36 KiB tiles, TWO workgroups = 32 waves
    //    per CU (picked automatically for small alphabets, m < 10)
    SLOT(24, BMX_TILE_F(1024, 68, 2, 3)); // 24: PRODUCT -- default geometry, 4-gram walker (picked automatically for
    //     small alphabets, m >= 10)
    SLOT(25, BMX_TILE_F(1024, 36, 2, 3)); // 25: PRODUCT -- 4-gram walker, 36 KiB tiles, two workgroups per CU
    SLOT(29, BMX_TILE_F(1024, 76, 2, 0)); // 29: PRODUCT -- 76 KiB tiles, room for 512 parked matches only (picked
    //     automatically for patterns over more than 8 distinct symbols, m >= 4)
    SLOT(53, BMX_TILE_S(1024, 76, 2, 10)); // 53: PRODUCT -- 76 KiB tiles, 8-gram walker (m >= 8), static shares + a stolen tail
    SLOT(54, BMX_TILE_S(1024, 76, 2, 3)); // 54: PRODUCT -- 76 KiB tiles, 4-gram walker, static shares + a stolen tail (ACGT, m = 8: +2 %)
    SLOT(79, BMX_TILE_S(1024, 76, 2, 0)); // 79: PRODUCT -- variant 29 with a stolen tail (scan_kernel MODE 12): long patterns on large alphabets
    SLOT(82, BMX_TILE_W32(1024, 36, 2, 12, 2)); // 82: PRODUCT -- variant 2 (skip loop, two workgroups per CU) with a stolen tail: large alphabets, m = 9..12
    SLOT(87, BMX_TILE_S(1024, 76, 2, 7)); // 87: PRODUCT (round 3) -- 76 KiB tiles, quad-SAD skip loop on the pattern's last 4 bytes (m < 4: the whole
    //     pattern), static shares + a stolen tail: texts over large alphabets, canonical tables, m >= 3 (config 2's kernel)
    SLOT(88, BMX_TILE_S(1024, 76, 2, 8)); // 88: PRODUCT (round 3) -- the same on the pattern's last 8 bytes (m >= 8): texts over 4..8 symbols (DNA), m = 8..15,
    //     where the 8-gram walker's shifts (m - 7) are still short (4 GiB ACGT, ms, 8-gram / this: m = 9: 1.56 / 0.70, m = 12: 0.86 / 0.69, m = 16: 0.68 / 0.69)
