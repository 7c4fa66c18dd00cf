/*
 * Stand-in for <glog/logging.h>, written for this project: just enough of the logging macros for the reference's
 * sources to compile where glog itself is absent.  Messages below FATAL are dropped; CHECK* and LOG(FATAL) print their
 * message and abort; DCHECK* compile their operands and evaluate nothing.
 *
 * TEST INFRASTRUCTURE ONLY (oracle/Makefile target `ref_full`).
 */
#ifndef RPF_ORACLE_GLOG_STAND_IN_H
#define RPF_ORACLE_GLOG_STAND_IN_H

#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

namespace glog_stand_in {

struct Sink {
    template <typename T>
    const Sink &operator<<(const T &) const { return *this; }
    const Sink &operator<<(std::ostream &(*)(std::ostream &)) const { return *this; }
};

class Fatal {
  public:
    Fatal(const char *file, int line, const char *what) { text_ << file << ":" << line << ": " << what << " "; }
    [[noreturn]] ~Fatal() {
        std::cerr << text_.str() << std::endl;
        std::abort();
    }
    template <typename T>
    const Fatal &operator<<(const T &v) const {
        text_ << v;
        return *this;
    }
    const Fatal &operator<<(std::ostream &(*f)(std::ostream &)) const {
        text_ << f;
        return *this;
    }

  private:
    mutable std::ostringstream text_;
};

/* gives both arms of the ?: in the macros below the type void, whatever was streamed */
struct Voidify {
    void operator&(const Sink &) const {}
    void operator&(const Fatal &) const {}
};

template <typename T>
T *check_not_null(const char *file, int line, const char *what, T *p) {
    if (p == nullptr) Fatal(file, line, what);
    return p;
}

}  // namespace glog_stand_in

#define GLOG_STAND_IN_SINK() (true) ? (void)0 : glog_stand_in::Voidify() & glog_stand_in::Sink()
#define GLOG_STAND_IN_INFO GLOG_STAND_IN_SINK()
#define GLOG_STAND_IN_WARNING GLOG_STAND_IN_SINK()
#define GLOG_STAND_IN_ERROR GLOG_STAND_IN_SINK()
#define GLOG_STAND_IN_FATAL glog_stand_in::Voidify() & glog_stand_in::Fatal(__FILE__, __LINE__, "LOG(FATAL)")

#define LOG(severity) GLOG_STAND_IN_##severity
#define LOG_IF(severity, cond) (!(cond)) ? (void)0 : GLOG_STAND_IN_##severity
#define VLOG(level) GLOG_STAND_IN_SINK()
#define VLOG_IS_ON(level) (false)

#define CHECK(cond) \
    (cond) ? (void)0 : glog_stand_in::Voidify() & glog_stand_in::Fatal(__FILE__, __LINE__, "Check failed: " #cond)
#define CHECK_EQ(a, b) CHECK((a) == (b))
#define CHECK_NE(a, b) CHECK((a) != (b))
#define CHECK_LT(a, b) CHECK((a) < (b))
#define CHECK_LE(a, b) CHECK((a) <= (b))
#define CHECK_GT(a, b) CHECK((a) > (b))
#define CHECK_GE(a, b) CHECK((a) >= (b))
#define CHECK_NOTNULL(p) glog_stand_in::check_not_null(__FILE__, __LINE__, "Check failed: '" #p "' must be non-null", (p))

#define DCHECK(cond) (true || (cond)) ? (void)0 : glog_stand_in::Voidify() & glog_stand_in::Sink()
#define DCHECK_EQ(a, b) DCHECK((a) == (b))
#define DCHECK_NE(a, b) DCHECK((a) != (b))
#define DCHECK_LT(a, b) DCHECK((a) < (b))
#define DCHECK_LE(a, b) DCHECK((a) <= (b))
#define DCHECK_GT(a, b) DCHECK((a) > (b))
#define DCHECK_GE(a, b) DCHECK((a) >= (b))

namespace google {
inline void InitGoogleLogging(const char *) {}
}  // namespace google

static int FLAGS_stderrthreshold __attribute__((unused)) = 0;
static int FLAGS_minloglevel __attribute__((unused)) = 0;
static int FLAGS_v __attribute__((unused)) = 0;
static bool FLAGS_logtostderr __attribute__((unused)) = false;
static std::string FLAGS_log_dir __attribute__((unused));

#endif  // RPF_ORACLE_GLOG_STAND_IN_H
