/*
 * tx_ref_harness.cpp -- extern "C" entry points around the reference's own
 * transmit helpers, appended after the functions tests/test_tx_ref_cpu.py
 * extracts from the reference's cpuLS.hpp and behind tx_ref_standins.hpp.
 *
 * TEST INFRASTRUCTURE ONLY.  The cyclic-prefix length is the reference's
 * compile-time `prefix` macro: one build of this harness per prefix.
 */
extern "C" {

int tx_ref_prefix(void) { return prefix; }

/* ifftShiftOneRow (cpuLS.hpp:119-132) on row 0 of Y. */
void tx_ref_ifftshift(complexF *Y, int cols) { ifftShiftOneRow(Y, cols, 0); }

/* ifftOneRow (cpuLS.hpp:152-162) on row 0 of Y. */
void tx_ref_ifft(complexF *Y, int cols) { ifftOneRow(Y, cols, 0); }

/* addPrefix (cpuLS.hpp:391-398): Y rows x (cols + prefix) from dY rows x cols. */
void tx_ref_add_prefix(complexF *Y, complexF *dY, int rows, int cols) { addPrefix(Y, dY, rows, cols); }

/* modRefSymbol (cpuLS.hpp:466-489) on a given pilot file: Y gets cols + prefix
 * samples, X the cols - 1 rotated pilots. */
void tx_ref_mod_ref_symbol(complexF *Y, complexF *X, int cols, const char *path) {
    g_tx_pilot_path = path;
    modRefSymbol(Y, X, cols);
}

/* modOneSymbol (cpuLS.hpp:492-529) with chanMultiply = false: X users x
 * (cols - 1); Y (users x (cols + prefix), also the function's staging area)
 * receives the modulated rows. */
void tx_ref_mod_one_symbol(complexF *Y, complexF *X, int cols, int users) {
    modOneSymbol(Y, 0, X, users, cols, users, false);
}

}
